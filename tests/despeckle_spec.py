"""The despeckle pass as include/jade_bvh.h states it ("Despeckle, stated"), in numpy float32 with one rounding per operation.

despeckle(c, v, ...) -> (colour, variance | None, scale, report): every array float32, the report a dict of the four counts.
`variant` takes one of four deliberately WRONG statements, for the tests that show the cases can tell them from the true one:
  "centre"     the centre pixel counted among its own neighbours
  "replicate"  the border replicated (coordinates clamped) instead of skipped
  "rank"       the (K + 1)-th largest taken for the K-th
  "vscale"     v not scaled by k^2 on a clamped pixel
"""
import numpy as np

F = np.float32
VARIANTS = ("centre", "replicate", "rank", "vscale")
REPORT = ("n_usable", "n_above", "n_established", "n_clamped")


def luminance(c):
    """Y = (0.3f * r + 0.6f * g) + 0.1f * b, five float operations"""
    with np.errstate(all="ignore"):
        return (F(0.3) * c[..., 0] + F(0.6) * c[..., 1]) + F(0.1) * c[..., 2]


def usable(c):
    return np.isfinite(c).all(-1) & np.isfinite(luminance(c))


def kth_largest(y, ok, radius, rank, variant=None):
    """B of every pixel and whether N(p) holds at least `rank` pixels.  y [H, W] float32, ok [H, W] bool."""
    h, w = y.shape
    key = np.where(ok, y, -np.inf).astype(F)  # an unusable pixel is nobody's neighbour
    yy, xx = np.mgrid[0:h, 0:w]
    cols = []
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            if dx == 0 and dy == 0 and variant != "centre":
                continue
            qy, qx = yy + dy, xx + dx
            if variant == "replicate":
                cols.append(key[np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)])
            else:
                inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                cols.append(np.where(inside, key[np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)], F(-np.inf)))
    n = np.stack(cols, -1)
    k = rank + 1 if variant == "rank" else rank
    if k > n.shape[-1]:
        return np.full((h, w), -np.inf, F), np.zeros((h, w), bool)
    top = -np.sort(-n, -1)  # descending; ties stay separate entries
    b = top[..., k - 1]
    return b, b != -np.inf


def one_pass(c, v, scale, radius, rank, gain, floor, zz, variant=None):
    c = c.copy()
    v = None if v is None else v.copy()
    scale = scale.copy()
    with np.errstate(all="ignore"):
        y = luminance(c)
        ok = usable(c)
        b, have = kth_largest(y, ok, radius, rank, variant)
        bound = F(gain) * np.where(b > 0, b, F(0.0)).astype(F) + F(floor)
        above = ok & have & (y > bound)
        established = np.zeros_like(above)
        if v is not None:
            d = y - bound
            established = above & np.isfinite(v) & (v >= 0) & (d * d > F(zz) * v)
        clamped = above & ~established
        k = (bound / np.where(clamped, y, F(1.0))).astype(F)
        for ch in range(3):
            c[..., ch] = np.where(clamped, k * c[..., ch], c[..., ch])
        if v is not None and variant != "vscale":
            v = np.where(clamped, (k * k) * v, v).astype(F)
        scale = np.where(clamped, scale * k, scale).astype(F)
    return c, v, scale, int(above.sum()), int(established.sum()), int(clamped.sum())


def despeckle(c, v=None, iterations=1, radius=1, rank=2, gain=2.0, floor=0.0, sigmas=2.0, variant=None):
    c = np.ascontiguousarray(c, F).copy()
    v = None if v is None else np.ascontiguousarray(v, F).copy()
    assert c.ndim == 3 and c.shape[2] == 3 and (v is None or v.shape == c.shape[:2])
    assert 0 <= iterations <= 4 and 1 <= radius <= 3 and 1 <= rank <= 4 and variant in (None,) + VARIANTS
    zz = F(sigmas) * F(sigmas)
    scale = np.ones(c.shape[:2], F)
    report = dict.fromkeys(REPORT, 0)
    report["n_usable"] = int(usable(c).sum())
    for _ in range(iterations):
        c, v, scale, a, e, k = one_pass(c, v, scale, radius, rank, gain, floor, zz, variant)
        report["n_above"] += a
        report["n_established"] += e
        report["n_clamped"] += k
    return c, v, scale, report
