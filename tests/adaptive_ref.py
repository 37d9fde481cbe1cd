"""numpy statement of the adaptive-sampling pixel error (include/jade_bvh.h, jade_render_adaptive / jade_render_error)."""
import numpy as np

LANES = 1024  # JADE_SAMPLE_LANES


def lane_sums(samples):
    """Per-sample radiance [n, ..., 3] float32 -> the lane sums [K, ..., 3] float32 a render of n samples keeps: sample s adds into
    lane s % 1024, in increasing s, in float32 (jade_rt.h)."""
    x = np.asarray(samples, np.float32)
    n = x.shape[0]
    k = min(n, LANES)
    out = np.zeros((k,) + x.shape[1:], np.float32)
    for s in range(n):
        out[s % LANES] = out[s % LANES] + x[s]
    return out


def pixel_error(lanes, n, error_floor):
    """lanes [K, ..., 3] (K = min(n, 1024)) of pixels with n samples -> float32 [...]:
        Y_l = (0.3 S_l.r + 0.6 S_l.g + 0.1 S_l.b) / c,  c = n / K
        m   = (1/K) sum Y_l
        err = sqrt( sum (Y_l - m)^2 / (K (K - 1)) ) / (m + error_floor)
    in fp64; NaN where n cannot be estimated (n < 2, or n > 1024 and not a multiple of 1024)."""
    s = np.asarray(lanes, np.float64)
    if n < 2 or (n > LANES and n % LANES):
        return np.full(s.shape[1:-1], np.nan, np.float32)
    k = min(n, LANES)
    assert s.shape[0] == k
    c = n // k
    y = (0.3 * s[..., 0] + 0.6 * s[..., 1] + 0.1 * s[..., 2]) / c
    m = y.sum(axis=0) / k
    var = ((y - m) ** 2).sum(axis=0) / (k * (k - 1))
    return (np.sqrt(var) / (m + error_floor)).astype(np.float32)


def tile_errors(err_map, tiles_x, tiles_y):
    """[H, W] pixel errors -> [tiles_y, tiles_x] maxima over each tile's in-image pixels (NaN counts as not converged: +inf)."""
    e = np.where(np.isnan(err_map), np.inf, err_map)
    out = np.zeros((tiles_y, tiles_x), np.float32)
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            out[ty, tx] = e[ty * 16:(ty + 1) * 16, tx * 16:(tx + 1) * 16].max()
    return out
