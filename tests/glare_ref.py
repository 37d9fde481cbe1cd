"""The glare of include/jade_bvh.h stated in numpy: float64 by default, `dtype=np.float32` to evaluate the same statement in the
device's number format (every product and every sum rounded to dtype, in the header's order)."""
import numpy as np

H5 = (1.0 / 16.0, 4.0 / 16.0, 6.0 / 16.0, 4.0 / 16.0, 1.0 / 16.0)  # exact in either format
TOL = 1e-5  # relative L2 of the device against the float64 statement (tests/test_gpu_glare.py says where it comes from)


def level_sizes(h, w, levels):
    """[(H_0, W_0), ..., (H_levels, W_levels)]: W_{k+1} = ceil(W_k / 2); a 1x1 level stays 1x1."""
    out = [(h, w)]
    for _ in range(levels):
        h, w = (h + 1) // 2, (w + 1) // 2
        out.append((h, w))
    return out


def weights(levels, falloff):
    """w_k = f^(k-1) / sum_j f^(j-1), k = 1 .. levels, in double."""
    w = np.float64(falloff) ** np.arange(levels, dtype=np.float64)
    return w / w.sum()


def reduce1(a, axis, dt):
    """REDUCE along one axis: out(x) = sum_i h(i) a(clamp(2x + i)), i = -2 .. 2 added in increasing i."""
    a = np.moveaxis(a, axis, 0)
    n = a.shape[0]
    x = np.arange((n + 1) // 2)
    acc = np.zeros((len(x),) + a.shape[1:], dt)
    for i in range(-2, 3):
        acc = (acc + (dt(H5[i + 2]) * a[np.clip(2 * x + i, 0, n - 1)]).astype(dt)).astype(dt)
    return np.moveaxis(acc, 0, axis)


def reduce(a, dt=np.float64):
    """L_k -> L_{k+1}: rows (x, axis 1) first, then columns (y, axis 0)."""
    return reduce1(reduce1(a, 1, dt), 0, dt)


def expand1(a, n, axis, dt):
    """EXPAND along one axis to n entries; source indices clamped to [0, m-1]."""
    a = np.moveaxis(a, axis, 0)
    m = a.shape[0]
    x = np.arange(n)
    j = x // 2
    lo, mid, hi = a[np.clip(j - 1, 0, m - 1)], a[np.clip(j, 0, m - 1)], a[np.clip(j + 1, 0, m - 1)]
    even = (((dt(0.125) * lo).astype(dt) + (dt(0.75) * mid).astype(dt)).astype(dt) + (dt(0.125) * hi).astype(dt)).astype(dt)
    odd = ((dt(0.5) * mid).astype(dt) + (dt(0.5) * hi).astype(dt)).astype(dt)
    sel = (x % 2 == 0).reshape((n,) + (1,) * (a.ndim - 1))
    return np.moveaxis(np.where(sel, even, odd), 0, axis)


def expand(a, h, w, dt=np.float64):
    """To h x w: rows (y, axis 0) first, then columns (x, axis 1)."""
    return expand1(expand1(a, h, 0, dt), w, 1, dt)


def glare(rgb, levels=6, strength=0.1, falloff=0.5, dtype=np.float64):
    """out_rgb of jade_glare_image for rgb [H, W, 3], in `dtype`."""
    dt = dtype
    rgb = np.asarray(rgb)
    if strength == 0:
        return rgb.copy()
    bad = ~np.isfinite(rgb).all(-1)
    L = [np.where(bad[..., None], 0, rgb).astype(dt)]
    for _ in range(levels):
        L.append(reduce(L[-1], dt))
    w = weights(levels, falloff)
    A = (dt(w[levels - 1]) * L[levels]).astype(dt)
    for k in range(levels - 1, 0, -1):
        h, wd = L[k].shape[:2]
        A = ((dt(w[k - 1]) * L[k]).astype(dt) + expand(A, h, wd, dt)).astype(dt)
    h, wd = rgb.shape[:2]
    s = np.float32(strength)
    one_minus_s = np.float32(1.0) - s  # one float subtraction, as the library's
    out = ((dt(one_minus_s) * L[0]).astype(dt) + (dt(s) * expand(A, h, wd, dt)).astype(dt)).astype(dt)
    return np.where(bad[..., None], rgb, out)
