"""One-light sampling (jade_scene_set_light_sampling = JADE_LIGHTS_ONE), stated independently in numpy.

Written from the text of include/jade_bvh.h ("The lights, stated"), not from light_alias_table (jade_scene_prep.hip) or light_sample
(jade_shade.h):

  * weights(tri, emit):        the distribution p over the entries of emit_indices the table is to realise;
  * draw(table, u1..u4):       entry, own, folded (rx, ry), q and weight of one draw, in float64;
  * draw_f32(table, u1..u4):   the same with the header's fp32 operations - what the device must give bit for bit.

Everything is float64 except what the header defines in fp32: the area a_i (the integrator's own tri_size), the slot product
fl(u1 * fl(nE)), the fold of (rx, ry) and the weight fl(fl(nE) / q).  The table's records, how a table's implied distribution is read off
and the pairing used to exercise the checks without the module are those of tests/env_importance_spec.py: the two modes share the
builder, and the header gives both tables the same meaning."""
import numpy as np

from env_importance_spec import TABLE, alias_counts, build_table, implied, slot_of  # noqa: F401  (re-exported for the tests)

MAX_ENTRIES = 1 << 24  # JADE_LIGHTS_ONE_MAX_ENTRIES


def tri_size_f32(tf):
    """a [n] float32: 0.5f * sqrt(dot(c, c)), c = cross(p2 - p1, p3 - p1), one fp32 operation each (PathTrace.cu:897-903), of the triangle
    rows tf [n, 28] (words 1-9 the vertices)."""
    tf = np.asarray(tf, np.float32)
    p1, p2, p3 = tf[:, 1:4], tf[:, 4:7], tf[:, 7:10]
    with np.errstate(all="ignore"):
        b, c = p2 - p1, p3 - p1
        # jv_cross (include/jade_fpmath.h): each component a difference of two rounded products
        cx = b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1]
        cy = b[:, 2] * c[:, 0] - b[:, 0] * c[:, 2]
        cz = b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0]
        d = (cx * cx + cy * cy) + cz * cz
        return np.float32(0.5) * np.sqrt(d)


def weights(tf, emit):
    """p [nE], float64: the probability of each entry of emit (indices into the triangle rows tf [n, 28]; words 13-15 the emission)."""
    tf = np.asarray(tf, np.float32)
    emit = np.asarray(emit, np.int64)
    n = len(emit)
    a = tri_size_f32(tf[emit]).astype(np.float64)
    a = np.where(np.isfinite(a), a, 0.0)
    e = tf[emit, 13:16].astype(np.float64)
    with np.errstate(all="ignore"):
        c = np.where(e < 0, 0.0, e)  # max(c, 0); a NaN stays a NaN
        lum = 0.2126 * c[:, 0] + 0.7152 * c[:, 1] + 0.0722 * c[:, 2]
        lum = np.where(np.isfinite(lum), lum, 0.0)
        w = a * lum
    w = np.where(np.isfinite(w), w, 0.0)
    total = w.sum()
    floor = 0.01 * total / n if total > 0 else 1.0
    w = w + floor
    return w / w.sum()


def fold(u3, u4):
    """(rx, ry) float32 as the reference folds them: rx + ry > 1 (the sum in fp32) -> (1 - rx, 1 - ry)."""
    rx, ry = np.asarray(u3, np.float32), np.asarray(u4, np.float32)
    over = (rx + ry) > np.float32(1)
    return np.where(over, np.float32(1) - rx, rx), np.where(over, np.float32(1) - ry, ry)


def draw(table, u1, u2, u3, u4):
    """One draw per row of the fp32 uniforms -> (entry int64 [n], own bool [n], rx, ry float32 [n], q float64 [n], weight float64 [n])."""
    n = len(table)
    assert 1 <= n <= MAX_ENTRIES
    s = slot_of(u1, n)
    e = table[s]
    own = np.asarray(u2, np.float32).astype(np.float64) < e["accept"].astype(np.float64)
    entry = np.where(own, s, e["alias"].astype(np.int64))
    q = np.where(own, e["q_own"], e["q_alias"]).astype(np.float64)
    rx, ry = fold(u3, u4)
    return entry, own, rx, ry, q, float(n) / q


def draw_f32(table, u1, u2, u3, u4):
    """... with weight = fl(fl(nE) / q): (entry, own, rx, ry, weight float32)."""
    entry, own, rx, ry, q, _ = draw(table, u1, u2, u3, u4)
    return entry, own, rx, ry, np.float32(len(table)) / q.astype(np.float32)


def estimator_mean(table, f):
    """(1 / nE) sum over slots s of [accept_s f(s) nE / q_own_s + (1 - accept_s) f(alias_s) nE / q_alias_s]: the expectation of
    weight x f(entry) over the slot and the own / alias draw, in float64 on the table's fp32 entries."""
    n = len(table)
    f = np.asarray(f, np.float64)
    acc = table["accept"].astype(np.float64)
    own = acc * f * n / table["q_own"].astype(np.float64)
    other = (1.0 - acc) * f[table["alias"]] * n / table["q_alias"].astype(np.float64)
    return (own + other).sum() / n


# ------------------------------------------------------------------ shared test inputs

def triangles(n, seed):
    """n triangle rows [n, 28] float32 with random vertices in a box and no emission."""
    rng = np.random.default_rng(seed)
    tf = np.zeros((n, 28), np.float32)
    tf[:, 1:10] = (rng.random((n, 9)) * 4 - 2).astype(np.float32)
    return tf


def emitter_list(kind):
    """(tf [n, 28] float32, emit int32 [nE]) for the cases the table is checked on."""
    rng = np.random.default_rng(77)
    if kind in ("one", "two", "three"):
        n = {"one": 1, "two": 2, "three": 3}[kind]
        tf = triangles(5, 1)
        tf[:n, 13:16] = (rng.random((n, 3)) * 30 + 1).astype(np.float32)
        return tf, np.arange(n, dtype=np.int32)
    if kind == "unequal82":       # 80 small dim triangles and two large bright ones: q spans five orders of magnitude
        tf = triangles(90, 2)
        tf[:80, 1:10] *= np.float32(0.05)
        tf[:80, 13:16] = (rng.random((80, 3)) * 2 + 0.1).astype(np.float32)
        tf[80:82, 13:16] = np.float32([[400, 380, 300], [90, 120, 150]])
        return tf, np.arange(82, dtype=np.int32)
    if kind == "duplicates":      # entries 0, 3 and 5 name one triangle: three separate entries of equal probability
        tf = triangles(6, 3)
        tf[:4, 13:16] = (rng.random((4, 3)) * 10 + 1).astype(np.float32)
        return tf, np.int32([0, 1, 2, 0, 3, 0, 2])
    if kind == "non-emitter":     # triangle 4 is listed and does not emit: the floor alone
        tf = triangles(6, 4)
        tf[:4, 13:16] = (rng.random((4, 3)) * 10 + 1).astype(np.float32)
        return tf, np.int32([0, 4, 1, 2, 3])
    if kind == "nan-channel":     # a NaN channel, an infinite one, a negative one, a degenerate triangle with huge emission
        tf = triangles(7, 5)
        tf[:6, 13:16] = (rng.random((6, 3)) * 10 + 1).astype(np.float32)
        tf[1, 14] = np.nan
        tf[2, 13] = np.inf
        tf[3, 15] = -5.0
        tf[4, 4:10] = tf[4, 1:4].tolist() * 2
        tf[4, 13:16] = 3e38
        return tf, np.arange(6, dtype=np.int32)
    if kind == "zero-power":      # nothing listed emits: every entry equally likely
        tf = triangles(9, 6)
        return tf, np.int32([8, 1, 2, 5])
    raise ValueError(kind)


KINDS = ("one", "two", "three", "unequal82", "duplicates", "non-emitter", "nan-channel", "zero-power")


def table_of(lib, tf, emit):
    """jade_debug_light_table_host (libjade_hip_debug.so; no HIP call) on triangle rows tf [n, 28] and emit [nE]: TABLE records [nE]."""
    import ctypes as C
    fn = lib.jade_debug_light_table_host
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    tf = np.ascontiguousarray(tf, np.float32)
    assert tf.shape[1] == 28
    emit = np.ascontiguousarray(emit, np.int32)
    out = np.zeros(max(len(emit), 1), TABLE)
    rc = fn(tf.ctypes.data, len(tf), emit.ctypes.data, len(emit), out.ctypes.data)
    assert rc == 0, rc
    return out[:len(emit)]


def sample_device(scene, u):
    """jade_debug_light_sample on float32 uniforms u [n, 4] over the scene's own table: (entry int64 [n], rx, ry float32 [n], the draw's
    weight float32 [n], light_weight of the entry float32 [n])."""
    import ctypes as C
    fn = scene.backend.lib.jade_debug_light_sample
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 4
    u = np.ascontiguousarray(u, np.float32)
    e = np.full(len(u), 0xffffffff, np.uint32)
    xy = np.full((len(u), 2), np.nan, np.float32)
    w = np.full((len(u), 2), np.nan, np.float32)
    scene.backend.check(fn(scene._h, len(u), u.ctypes.data, e.ctypes.data, xy.ctypes.data, w.ctypes.data))
    return e.astype(np.int64), xy[:, 0], xy[:, 1], w[:, 0], w[:, 1]
