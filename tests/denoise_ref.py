"""float64 numpy statement of the denoiser (include/jade_bvh.h: jade_render_denoise / jade_denoise_image / jade_render_guides).

The variance input comes from adaptive_ref's estimator: the pixel error's numerator, squared."""
import numpy as np

from adaptive_ref import pixel_error

H5 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])
G3 = np.array([1 / 4, 1 / 2, 1 / 4])


def luminance(c):
    return 0.3 * c[..., 0] + 0.6 * c[..., 1] + 0.1 * c[..., 2]


def pixel_variance(lanes, n):
    """lanes [K, ..., 3] of pixels with n samples -> variance of the mean luminance, sum (Y_l - m)^2 / (K (K - 1)): adaptive_ref's
    pixel error times (m + floor), squared; NaN where n cannot be estimated.  (float64 from the float32 error: ~1e-7 relative.)"""
    floor = 1.0
    err = pixel_error(lanes, n, floor).astype(np.float64)
    m = luminance(np.asarray(lanes, np.float64).sum(axis=0)) / n
    return (err * (m + floor)) ** 2


def _shift(a, oy, ox):
    """b[y, x] = a[y + oy, x + ox] where that is in the image; (b, valid)."""
    h, w = a.shape[:2]
    b = np.zeros_like(a)
    ok = np.zeros((h, w), bool)
    y0, y1 = max(0, -oy), min(h, h - oy)
    x0, x1 = max(0, -ox), min(w, w - ox)
    if y0 < y1 and x0 < x1:
        b[y0:y1, x0:x1] = a[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
        ok[y0:y1, x0:x1] = True
    return b, ok


def unusable(rgb, variance, albedo, normal, depth):
    """[H, W] bool: the pixels the filter leaves alone and never taps (include/jade_bvh.h, "Unusable pixels"): a non-finite channel of
    colour, albedo or normal, a non-finite depth, a non-finite or negative variance.  Decided once, from the inputs."""
    c, a, n = (np.asarray(x, np.float64) for x in (rgb, albedo, normal))
    v, z = np.asarray(variance, np.float64), np.asarray(depth, np.float64)
    with np.errstate(invalid="ignore"):
        return ~(np.isfinite(c).all(-1) & np.isfinite(a).all(-1) & np.isfinite(n).all(-1) & np.isfinite(z) & np.isfinite(v) & (v >= 0))


def unit_normals(n, zero):
    """nhat = n / |n| of every non-zero normal whatever its length: n is first scaled by the power of two that brings its largest
    component into [1, 2) (exact), so that no square leaves the range of the type; 0 where `zero`."""
    dt = n.dtype.type
    m = np.abs(n).max(axis=-1)
    _, e = np.frexp(np.where(zero, dt(1), m))
    u = np.ldexp(np.where(zero[..., None], dt(0), n), (1 - e)[..., None]).astype(dt)
    length = np.sqrt((u * u).sum(axis=-1))
    return np.where(zero[..., None], dt(0), u / np.where(zero, dt(1), length)[..., None]).astype(dt)


def denoise(rgb, variance, albedo, normal, depth, iterations, sigma_l, sigma_n, sigma_z, sigma_a, dtype=np.float64):
    """[H, W, 3] rgb / albedo / normal, [H, W] variance / depth -> (filtered rgb [H, W, 3], filtered variance [H, W]), in `dtype`:
    float64 is the statement, float32 the same statement with every operation in float (what a float kernel can be expected to
    reach).  Unusable pixels (above) come back as they went in and are no tap of any sum."""
    dt = np.dtype(dtype).type
    c0 = np.asarray(rgb, dt)
    v0 = np.asarray(variance, dt)
    bad = unusable(rgb, variance, albedo, normal, depth)
    use = ~bad
    # (what an unusable pixel holds is never read below: finite stand-ins keep the arithmetic quiet)
    c = np.where(bad[..., None], dt(0), c0)
    v = np.where(bad, dt(0), v0)
    a = np.where(bad[..., None], dt(0), np.asarray(albedo, dt))
    n = np.where(bad[..., None], dt(0), np.asarray(normal, dt))
    z = np.where(bad, dt(0), np.asarray(depth, dt))
    h5, g3 = H5.astype(dt), G3.astype(dt)
    sigma_l, sigma_n, sigma_z, sigma_a, eps = dt(sigma_l), dt(sigma_n), dt(sigma_z), dt(sigma_a), dt(1e-10)
    zero = np.all(n == 0, axis=-1)
    nh = unit_normals(n, zero)
    for i in range(iterations):
        s = 1 << i
        gs = np.zeros_like(v)
        gw = np.zeros_like(v)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                vq, ok = _shift(v, dy, dx)
                ok &= _shift(use, dy, dx)[0]
                w = (g3[dy + 1] * g3[dx + 1]) * ok.astype(dt)
                gs += w * np.where(ok, vq, dt(0))
                gw += w
        g = gs / np.where(bad, dt(1), gw)
        lp = luminance(c).astype(dt)
        sw = np.zeros_like(v)
        sc = np.zeros_like(c)
        sv = np.zeros_like(v)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                cq, ok = _shift(c, s * dy, s * dx)
                ok &= _shift(use, s * dy, s * dx)[0]
                vq, _ = _shift(v, s * dy, s * dx)
                aq, _ = _shift(a, s * dy, s * dx)
                nq, _ = _shift(nh, s * dy, s * dx)
                zq, _ = _shift(z, s * dy, s * dx)
                zeroq, _ = _shift(zero, s * dy, s * dx)
                wl = np.exp(-np.abs(lp - luminance(cq).astype(dt)) / (sigma_l * np.sqrt(g) + eps))
                dot = (nh * nq).sum(axis=-1)
                wn = np.where(zero & zeroq, dt(1), np.where(zero | zeroq, dt(0), np.maximum(dot, dt(0)) ** sigma_n))
                wz = np.exp(-np.abs(z - zq) / (sigma_z * np.maximum(z, zq) + eps))
                wa = np.exp(-np.abs(a - aq).sum(axis=-1) / sigma_a)
                w = np.where(ok, h5[dx + 2] * h5[dy + 2] * wl * wn * wz * wa, dt(0)).astype(dt)
                sw += w
                sc += w[..., None] * np.where(ok[..., None], cq, dt(0))
                sv += w * w * np.where(ok, vq, dt(0))
        sw = np.where(bad, dt(1), sw)
        c = (sc / sw[..., None]).astype(dt)
        v = (sv / (sw * sw)).astype(dt)
    return np.where(bad[..., None], c0, c), np.where(bad, v0, v)
