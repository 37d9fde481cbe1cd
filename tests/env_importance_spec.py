"""Environment importance sampling (jade_render_params.env_sampling = JADE_ENV_IMPORTANCE), stated independently in float64 numpy.

Written from the text of include/jade_rt.h (at JADE_ENV_IMPORTANCE) and from tests/env_spec.py's statement of SampleSphericalMap,
not from env_alias_table (jade_scene_prep.hip) or env_sample (jade_shade.h):

  * weights(env, W, H): the distribution p over the texels the table is to realise;
  * implied(table):     the distribution P a table {accept, alias, q_own, q_alias} DOES realise, whoever paired its texels;
  * draw(table, W, H, u1..u4): texel, own, direction and ratio of one draw.

Everything is float64 except the slot product fl(u1 * fl(N)), a discrete decision the header defines in fp32, and the two angle
constants fl(PI) and fl(2 PI), which the header names as such.  How small texels are paired with large ones (Vose's method in the
module) is not part of the statement: draw() takes the table as data."""
import numpy as np

PI = 3.1415926  # #define PI, PathTrace.cu:36
PI_F = float(np.float32(PI))
TWO_PI_F = float(np.float32(2.0 * PI))
MAX_TEXELS = 1 << 24  # JADE_ENV_IMPORTANCE_MAX_TEXELS

TABLE = np.dtype([("accept", np.float32), ("alias", np.uint32), ("q_own", np.float32), ("q_alias", np.float32)])


def weights(env, w, h):
    """p [N], float64: the probability of each texel (row-major, row 0 on top) of env [H, W, 3]."""
    env = np.asarray(env, np.float64).reshape(h, w, 3)
    with np.errstate(all="ignore"):
        c = np.where(env < 0, 0.0, env)  # max(c, 0); a NaN stays a NaN
        lum = 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]
    lum = np.where(np.isfinite(lum), lum, 0.0)
    total = lum.sum()
    floor = 0.01 * total / (w * h) if total > 0 else 1.0
    row_sine = np.sin(PI * (np.arange(h) + 0.5) / h)
    wgt = (lum + floor) * row_sine[:, None]
    return (wgt / wgt.sum()).ravel()


def implied(table):
    """P [N], float64: the probability with which a draw from `table` (TABLE records) returns each texel."""
    n = len(table)
    acc = table["accept"].astype(np.float64)
    away = np.where(table["alias"] != np.arange(n), 1.0 - acc, 0.0)  # what slot s sends to another texel
    own = np.where(table["alias"] != np.arange(n), acc, 1.0)         # (a slot that is its own alias keeps everything)
    return (own + np.bincount(table["alias"], weights=away, minlength=n)) / n


def alias_counts(table):
    """m [N]: the number of OTHER slots whose alias is each texel."""
    n = len(table)
    other = table["alias"] != np.arange(n)
    return np.bincount(table["alias"][other], minlength=n)


def slot_of(u1, n):
    """min((uint32)fl(u1 * fl(N)), N - 1): the only fp32 arithmetic of the statement."""
    prod = np.asarray(u1, np.float32) * np.float32(n)
    return np.minimum(prod.astype(np.int64), n - 1)


def direction_of(u, v):
    """(direction [n, 3], sin(theta) clamped at 0) of the map point (u, v): the inverse of env_spec.uv_of with the header's constants."""
    theta = PI_F * np.asarray(v, np.float64)
    phi = TWO_PI_F * (np.asarray(u, np.float64) - 0.5)
    st = np.maximum(np.sin(theta), 0.0)
    return np.stack([st * np.cos(phi), np.cos(theta), st * np.sin(phi)], -1), st


def draw(table, w, h, u1, u2, u3, u4):
    """One draw per row of the fp32 uniforms u1..u4 -> (texel int64 [n], own bool [n], direction float64 [n, 3], ratio float64 [n],
    q float64 [n])."""
    n = w * h
    assert len(table) == n and n <= MAX_TEXELS
    u2, u3, u4 = (np.asarray(x, np.float32).astype(np.float64) for x in (u2, u3, u4))
    s = slot_of(u1, n)
    e = table[s]
    own = u2 < e["accept"].astype(np.float64)
    texel = np.where(own, s, e["alias"].astype(np.int64))
    q = np.where(own, e["q_own"], e["q_alias"]).astype(np.float64)
    j, i = np.divmod(texel, w)
    d, st = direction_of((i + u3) / w, (j + u4) / h)
    return texel, own, d, PI_F * st / q, q


def build_table(p):
    """A table for p by a pairing of this file's own (smallest with largest, by a sort): used to exercise implied() and draw() without
    the module, and as evidence that the checks do not depend on Vose's order."""
    n = len(p)
    q = np.asarray(p, np.float64) * n
    t = np.zeros(n, TABLE)
    t["alias"] = np.arange(n)
    t["accept"] = 1.0
    r = q.copy()
    small = [i for i in np.argsort(q) if q[i] < 1.0]
    large = [i for i in np.argsort(-q) if q[i] >= 1.0]
    while small and large:
        a, g = small.pop(0), large[0]
        t["accept"][a] = np.float32(r[a])
        t["alias"][a] = g
        r[g] = (r[g] + r[a]) - 1.0
        if r[g] < 1.0:
            large.pop(0)
            small.append(g)
    t["q_own"] = q.astype(np.float32)
    t["q_alias"] = q[t["alias"]].astype(np.float32)
    return t


# ------------------------------------------------------------------ shared test inputs

MAP_SIZES = ((1, 1), (1, 4), (5, 1), (2, 2), (7, 5), (64, 32), (257, 3))  # (W, H)
KINDS = ("random", "constant", "black", "hot", "nonfinite")


def make_map(w, h, kind):
    """float32 [H, W, 3].  random: env_spec.make_map's texels; constant: every q equal within a row; black: the floor alone; hot: one
    texel at 1e6 on black; nonfinite: random with NaN, +-inf and negative channels strewn in."""
    rng = np.random.default_rng(1000 * w + h)
    env = (rng.random((h, w, 3)) * 4.0).astype(np.float32)
    if kind == "random":
        env[rng.random((h, w, 3)) < 0.1] = 25.0
    elif kind == "constant":
        env[:] = (0.5, 0.6, 0.8)
    elif kind == "black":
        env[:] = 0.0
    elif kind == "hot":
        env[:] = 0.0
        env[(h - 1) // 3, (2 * w) // 3] = 1e6
    elif kind == "nonfinite":
        flat = env.reshape(-1)
        for k, val in enumerate((np.nan, np.inf, -np.inf, -3.0, -0.0, 3e38)):
            flat[(7 * k + 1) % flat.size] = val
    else:
        raise ValueError(kind)
    return env


def table_of(lib, env):
    """jade_debug_env_alias_host (libjade_hip_debug.so; no HIP call) on env [H, W, 3]: TABLE records [N]."""
    import ctypes as C
    fn = lib.jade_debug_env_alias_host
    fn.restype = C.c_int
    fn.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    env = np.ascontiguousarray(env, np.float32)
    h, w = env.shape[:2]
    out = np.zeros(w * h, TABLE)
    rc = fn(w, h, env.ctypes.data, out.ctypes.data)
    assert rc == 0, rc
    return out


def sample_device(scene, u):
    """jade_debug_env_sample on float32 uniforms u [n, 4]: (direction float32 [n, 3], ratio float32 [n], texel int64 [n], own bool [n])."""
    import ctypes as C
    fn = scene.backend.lib.jade_debug_env_sample
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 4
    u = np.ascontiguousarray(u, np.float32)
    d = np.full((len(u), 3), np.nan, np.float32)
    r = np.full(len(u), np.nan, np.float32)
    t = np.full(len(u), 0xffffffff, np.uint32)
    scene.backend.check(fn(scene._h, len(u), u.ctypes.data, d.ctypes.data, r.ctypes.data, t.ctypes.data))
    return d, r, (t & np.uint32(0x7fffffff)).astype(np.int64), (t >> np.uint32(31)) == 1


def sample_device_rng(scene, states):
    """jade_debug_env_sample_rng on uint32 RNG states [n]: (state after the draw uint32 [n], direction, ratio)."""
    import ctypes as C
    fn = scene.backend.lib.jade_debug_env_sample_rng
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 4
    s = np.ascontiguousarray(states, np.uint32)
    after = np.zeros_like(s)
    d = np.full((len(s), 3), np.nan, np.float32)
    r = np.full(len(s), np.nan, np.float32)
    scene.backend.check(fn(scene._h, len(s), s.ctypes.data, after.ctypes.data, d.ctypes.data, r.ctypes.data))
    return after, d, r


def wang(s):
    """fshader_render.fsh:82-98 on a uint32 array: the next state (which is also the number drawn)."""
    s = np.asarray(s, np.uint64)
    m = np.uint64(0xffffffff)
    s = ((s ^ np.uint64(61)) ^ (s >> np.uint64(16))) & m
    s = (s * np.uint64(9)) & m
    s = s ^ (s >> np.uint64(4))
    s = (s * np.uint64(0x27d4eb2d)) & m
    s = s ^ (s >> np.uint64(15))
    return s.astype(np.uint32)


def uniform_of(state):
    """jade_rand's value for the state it has just moved to: fl(fl(uint32) * 2^-32)."""
    return np.asarray(state, np.uint32).astype(np.float32) * np.float32(2.0 ** -32)
