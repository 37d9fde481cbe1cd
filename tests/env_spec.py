"""The environment lookup, stated independently in float64 numpy.

Written from the reference's text and from CUDA's documented texture fetch, not from the oracle or the HIP module:

  * SampleSphericalMap / sampleHdr, PathTrace.cu:686-702:
        uv = (atan2(v.z, v.x), asin(v.y)) of the NORMALISED direction;  u = uv.x / (2 PI) + 0.5;  v = 1 - (uv.y / PI + 0.5)
        colour = min(tex2D(u, v), 10)        with PI = 3.1415926 as the reference writes it (PathTrace.cu:36)
  * the texture objects, PathTrace.cu:1652-1665: normalised coordinates, cudaAddressModeMirror on both axes,
    cudaFilterModeLinear, one float plane per channel, row 0 of the image = row 0 of the array.
  * CUDA C Programming Guide, "Texture Fetching": with normalised coordinates in mirror mode a coordinate x becomes frac(x) when
    floor(x) is even and 1 - frac(x) when it is odd; it is then scaled by the extent N; linear filtering reads
        tex(x) = (1 - a) T[i] + a T[i + 1],   xB = x - 0.5,  i = floor(xB),  a = frac(xB)
    and a tap outside 0 .. N-1 is addressed by the same mode: in mirror mode tap -1 is texel 0 and tap N is texel N - 1.

Departures, on purpose: the hardware stores `a` in 9-bit fixed point; this statement (like both backends, which filter in
software) keeps full precision.  Nothing here rounds to fp32: what the fp32 code may differ by is the test's tolerance.
"""
import numpy as np

PI = 3.1415926  # #define PI, PathTrace.cu:36


def uv_of(dirs):
    """(u, v) texture coordinates of float directions [n, 3], float64.  Exactly at a pole (x = z = 0) the angle is 0, whatever the
    signs of the zeros: what atan2(+0, +0) is, and what jade_atan2f returns for all four sign pairs (IEEE and CUDA's atan2f give
    +-pi for x = -0: a kept departure of measure zero, see tests/test_env_spec.py's seam test)."""
    d = np.asarray(dirs, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        nv = d / np.sqrt((d * d).sum(1))[:, None]
        pole = (nv[:, 0] == 0) & (nv[:, 2] == 0)
        u = np.where(pole, 0.0, np.arctan2(nv[:, 2], nv[:, 0])) / (2.0 * PI) + 0.5
        v = 1.0 - (np.arcsin(np.clip(nv[:, 1], -1.0, 1.0)) / PI + 0.5)
    return u, v


def _mirror_coord(x):
    f = np.floor(x)
    frac = x - f
    return np.where(np.mod(f, 2.0) == 0.0, frac, 1.0 - frac)


def _taps(x, n):
    """Linear filtering along one axis of extent n: (i0, i1, a) with mirror addressing of the coordinate and of the taps."""
    xb = _mirror_coord(x) * n - 0.5
    i = np.floor(xb)
    a = xb - i
    i = i.astype(np.int64)

    def tap(t):  # mirror addressing of a texel index: ... 1 0 | 0 1 .. n-1 | n-1 n-2 ...
        m = np.mod(t, 2 * n)
        return np.where(m >= n, 2 * n - 1 - m, m)
    return tap(i), tap(i + 1), a


def fetch(env, u, v):
    """tex2D(u, v) of env [H, W, 3] for each channel, float64 [n, 3]."""
    env = np.asarray(env, np.float64)
    h, w = env.shape[:2]
    i0, i1, ax = _taps(np.asarray(u, np.float64), w)
    j0, j1, ay = _taps(np.asarray(v, np.float64), h)
    ax, ay = ax[:, None], ay[:, None]
    top = (1 - ax) * env[j0, i0] + ax * env[j0, i1]
    bot = (1 - ax) * env[j1, i0] + ax * env[j1, i1]
    return (1 - ay) * top + ay * bot


def sample_hdr(env, dirs):
    """sampleHdr(v) for float directions [n, 3] against env [H, W, 3]: float64 [n, 3].  Directions that do not normalise to a finite
    unit vector (zero, NaN, inf) give NaN rows: the reference leaves them to the hardware."""
    u, v = uv_of(dirs)
    ok = np.isfinite(u) & np.isfinite(v)
    out = np.full((len(u), 3), np.nan)
    out[ok] = np.minimum(fetch(env, u[ok], v[ok]), 10.0)
    return out


def direction_of(u, v):
    """A unit direction (float64) that SampleSphericalMap sends to (u, v): the inverse of the map above."""
    phi = (np.asarray(u, np.float64) - 0.5) * (2.0 * PI)
    theta = (0.5 - np.asarray(v, np.float64)) * PI
    return np.stack([np.cos(theta) * np.cos(phi), np.sin(theta), np.cos(theta) * np.sin(phi)], -1)


def tolerance(env):
    """What an fp32 evaluation may differ from this statement by: coordinate errors of a few fp32 ulps of u, v and of atan2 / asin
    move the sample point by at most about 2e-7 W texels (H along v); bilinear interpolation turns that into at most that share of the
    contrast between texels; the interpolation itself rounds at about 1e-6 of the largest texel."""
    env = np.asarray(env, np.float64)
    h, w = env.shape[:2]
    return 2e-7 * (w + h) * (env.max() - env.min()) + 1e-6 * np.abs(env).max()


# ------------------------------------------------------------------ shared test inputs

MAP_SIZES = ((1, 1), (1, 4), (5, 1), (2, 2), (7, 5), (64, 32))  # (W, H)


def make_map(w, h):
    """Random texels in [0, 4), about a tenth of them 25 so that the clamp at 10 is hit."""
    rng = np.random.default_rng(1000 * w + h)
    env = rng.random((h, w, 3)) * 4.0
    env[rng.random((h, w, 3)) < 0.1] = 25.0
    return env.astype(np.float32)


def directions(w, h):
    """(dirs float32 [n, 3], spec_ok bool [n]): the directions a lookup in a W x H map is tried on; spec_ok marks those this
    statement defines (the zero vector and non-finite directions are compared between the backends only)."""
    rng = np.random.default_rng(7)
    g = rng.normal(size=(20000, 3))
    g *= 10.0 ** rng.uniform(-3, 3, (20000, 1))
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    # texel centres and edges: u = k / (2W), k = 0 .. 2W; v likewise
    uu, vv = np.meshgrid(np.arange(2 * w + 1) / (2.0 * w), np.arange(2 * h + 1) / (2.0 * h))
    grid = direction_of(uu.ravel(), vv.ravel())
    seam = [(-1, 0, z) for z in (0.0, -0.0, 1e-45, -1e-45, 1e-7, -1e-7)]
    poles = [(x, y, 0) for y in (1, -1) for x in (0.0, 1e-20, -1e-20)]
    good = np.concatenate([g, axes, grid, np.array(seam), np.array(poles)]).astype(np.float32)
    nan, inf = np.nan, np.inf
    bad = np.array([(0, 0, 0), (-0.0, -0.0, -0.0), (nan, 0, 1), (0, nan, 1), (1, 0, nan), (nan, nan, nan), (inf, 0, 0), (0, inf, 0),
                    (0, 0, -inf), (inf, inf, inf), (-inf, 1, 2), (1e30, 1e30, 0), (1e-30, 0, 1e-30)], np.float32)
    dirs = np.concatenate([good, bad])
    ok = np.concatenate([np.ones(len(good), bool), np.zeros(len(bad), bool)])
    return dirs, ok


def camera_dirs(p, frame=0):
    """The camera ray of sample 0 of every pixel of params p, PathTrace.cu:1428-1437, in float64: [H, W, 3].  The two jitter draws come
    from jade_spec.wang_stream (shaders/fshader_render.fsh:82-98)."""
    import jade_spec
    m = np.asarray(list(p.camera), np.float64).reshape(4, 4)
    out = np.zeros((p.height, p.width, 3))
    for y in range(p.height):
        for x in range(p.width):
            rng = jade_spec.wang_stream(x, y, frame)
            lx = (-1 + 2.0 / p.width * (x + next(rng) - 0.5)) * (p.width / p.height)
            ly = -1 + 2.0 / p.height * (y + next(rng) - 0.5)
            vec = np.array([lx, ly, -1.5, 0.0])
            d = np.array([sum(m[c][r] * vec[c] for c in range(4)) for r in range(3)])
            out[y, x] = d / np.sqrt(d @ d)
    return out


CAMERA_POSES = ((0.0, 0.0), (0.0, 90.0), (0.0, 180.0), (0.0, 270.0), (80.0, 30.0), (-80.0, 200.0))  # (up_deg, rot_deg): all around, both poles


def sky_scene(env):
    """A scene that is all sky: the map env [H, W, 3] and one tiny triangle far behind every camera of CAMERA_POSES' orbit."""
    import jaderaytracerendering_amd as J
    from jaderaytracerendering_amd import host as H
    b = J.SceneBuilder()
    v = np.float32([[9000, 9000, 9000], [9000.001, 9000, 9000], [9000, 9000.001, 9000]])
    b.add_mesh(v, np.arange(3).reshape(1, 3), H.material(brdf=(0.5, 0.5, 0.5)))
    b.set_env_data(np.ascontiguousarray(env, np.float32))
    return b.build()


def sky_params(pose, width=24, height=16):
    """One sample per pixel from the orbit pose (up_deg, rot_deg), eye on the orbit of radius 4."""
    from jaderaytracerendering_amd import backend as B
    from jaderaytracerendering_amd import host as H
    eye, cam = H.camera_orbit(4.0, pose[0], pose[1])
    return B.make_params(width, height, 1, eye, cam, threads=2)


def lookup(scene, entry, dirs):
    """jade_oracle_sample_hdr (oracle) / jade_debug_sample_hdr (libjade_hip_debug.so) on float32 dirs [n, 3]: float32 [n, 3]."""
    import ctypes as C
    fn = getattr(scene.backend.lib, entry)
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    dirs = np.ascontiguousarray(dirs, np.float32)
    out = np.full((len(dirs), 3), -1.0, np.float32)
    scene.backend.check(fn(scene._h, len(dirs), dirs.ctypes.data, out.ctypes.data))
    return out
