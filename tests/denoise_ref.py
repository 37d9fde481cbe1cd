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


def denoise(rgb, variance, albedo, normal, depth, iterations, sigma_l, sigma_n, sigma_z, sigma_a):
    """[H, W, 3] rgb / albedo / normal, [H, W] variance / depth -> (filtered rgb [H, W, 3], filtered variance [H, W]), float64."""
    c = np.asarray(rgb, np.float64)
    v = np.asarray(variance, np.float64)
    a = np.asarray(albedo, np.float64)
    n = np.asarray(normal, np.float64)
    z = np.asarray(depth, np.float64)
    zero = np.all(n == 0, axis=-1)
    length = np.sqrt((n * n).sum(axis=-1))
    nh = np.where(zero[..., None], 0.0, n / np.where(zero, 1.0, length)[..., None])
    for i in range(iterations):
        s = 1 << i
        gs = np.zeros_like(v)
        gw = np.zeros_like(v)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                vq, ok = _shift(v, dy, dx)
                w = G3[dy + 1] * G3[dx + 1] * ok
                gs += w * np.where(ok, vq, 0.0)
                gw += w
        g = gs / gw
        lp = luminance(c)
        sw = np.zeros_like(v)
        sc = np.zeros_like(c)
        sv = np.zeros_like(v)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                cq, ok = _shift(c, s * dy, s * dx)
                vq, _ = _shift(v, s * dy, s * dx)
                aq, _ = _shift(a, s * dy, s * dx)
                nq, _ = _shift(nh, s * dy, s * dx)
                zq, _ = _shift(z, s * dy, s * dx)
                zeroq, _ = _shift(zero, s * dy, s * dx)
                wl = np.exp(-np.abs(lp - luminance(cq)) / (sigma_l * np.sqrt(g) + 1e-10))
                dot = (nh * nq).sum(axis=-1)
                wn = np.where(zero & zeroq, 1.0, np.where(zero | zeroq, 0.0, np.maximum(dot, 0.0) ** sigma_n))
                wz = np.exp(-np.abs(z - zq) / (sigma_z * np.maximum(z, zq) + 1e-10))
                wa = np.exp(-np.abs(a - aq).sum(axis=-1) / sigma_a)
                w = np.where(ok, H5[dx + 2] * H5[dy + 2] * wl * wn * wz * wa, 0.0)
                sw += w
                sc += w[..., None] * np.where(ok[..., None], cq, 0.0)
                sv += w * w * np.where(ok, vq, 0.0)
        c = sc / sw[..., None]
        v = sv / (sw * sw)
    return c, v
