"""Scenes that are legal under the C ABI (include/jade_rt.h: validate_desc checks ranges only) and unlike anything SceneBuilder makes.

One base scene - 148 triangles in six objects: a diffuse floor box, a jade geodesic of 80 triangles, a jade box, a DIR_REFRACT glass
box, a mirror box, a 20-triangle emissive geodesic, under a 16 x 8 sky - and its variants, each an edit of HostScene.a in place
(triangle words: 0 obj_idx, 1-9 vertices, 10-12 norm, 13-27 the material).  What SceneBuilder always delivers and a caller need not:
prefix_area a clean per-object running sum, index_mapping a permutation, one material per object, emit_indices exactly the emissive
triangles once each in ascending order, norm the unit face normal, obj_segs disjoint and in agreement with obj_idx.
jade_scene_create derives its guide tables, its material table and its emitter walk from exactly these arrays.

Also here, shared with tests/test_gpu_parity.py: the table of shading schedules under which a frame must be the same bits."""
import numpy as np

from jaderaytracerendering_amd import _abi, backend as B, host as H
from jaderaytracerendering_amd.host import HostScene

WIDTH, HEIGHT, SPP = 64, 48, 8
MAT = slice(13, 28)        # emissive[3] brdf[3] reflex_mode refract_mode refract_rate[3] refract_albedo[3] refract_index
EMISSIVE_BAR = 1.4e-5      # PathTrace.cu:916-920 (bounce_classify; the mirror chain's own test uses 1.5e-4)
JADE_OBJECTS = (1, 2)

# The schedules of test_gpu_parity.py::test_result_independent_of_shade_schedule: split, fused, batch, packet, budget, wide
# (k_trace_wide for the walk = 1 frame), tail (k_tail finishes short lists; 0: passes to the end), binned (k_shade deals its records
# by branch through LDS; 0: every thread runs its own record's whole bounce), records (k_trace refills from 48-B ray records the
# shading kernels wrote; 0: it gathers each ray through its queue entry)
SCHEDULE_KEYS = ("JADE_SHADE_SPLIT", "JADE_FUSED", "JADE_BATCH", "JADE_LIGHT_PACKET", "JADE_PACKET_BUDGET", "JADE_WIDE", "JADE_TAIL",
                 "JADE_SHADE_BINNED", "JADE_RAY_RECORDS")
SCHEDULES = (("1", "1", "1", "1", "32", "0", "1", "1", "1"), ("1", "1", "1", "0", "32", "1", "0", "1", "0"),
             ("1", "1", "1", "1", "3", "1", "1", "0", "1"), ("1", "1", "1", "1", "100000", "0", "0", "0", "0"),
             ("1", "0", "1", "1", "32", "1", "0", "1", "1"), ("0", "1", "1", "1", "32", "0", "1", "1", "0"),
             ("1", "1", "0", "1", "32", "1", "0", "1", "1"), ("1", "1", "0", "1", "32", "0", "1", "0", "0"),
             ("1", "0", "1", "1", "32", "0", "1", "0", "1"), ("0", "1", "0", "1", "32", "0", "0", "1", "1"))


def set_schedule(monkeypatch, values):
    for key, val in zip(SCHEDULE_KEYS, values):
        monkeypatch.setenv(key, val)


def _glass():
    return H.material(brdf=(0.05,) * 3, reflex_mode=_abi.MIRROR, refract_mode=_abi.DIR_REFRACT, refract_rate=(0.9, 0.95, 0.9),
                      refract_albedo=(0.3,) * 3, refract_index=1.5)


def _mirror():
    return H.material(brdf=(0.8, 0.8, 0.7), reflex_mode=_abi.MIRROR)


def _jade():
    return H.material(brdf=(0.3, 0.4, 0.5), reflex_mode=_abi.MIRROR, refract_mode=_abi.SUB_SURFACE, refract_rate=(0.3, 0.4, 0.5),
                      refract_albedo=(0.3, 0.5, 0.7), refract_index=2.66)


def _build(small_jade_last=False):
    b = H.SceneBuilder()
    try:
        T = H.transform_matrix
        b.add_proc("box", 0, H.material(brdf=(0.6, 0.5, 0.4)), T(trans=(0, -1.1, 0), scale=(7, 0.2, 7)))
        b.add_proc("geodesic", 2, _jade(), T(rot_deg=(10, 20, 0), trans=(-1.1, -0.25, 0.2), scale=(0.42,) * 3))
        b.add_proc("box", 0, _jade(), T(rot_deg=(0, 35, 0), trans=(0.45, -0.6, 1.0), scale=(0.8,) * 3))
        b.add_proc("box", 0, _glass(), T(rot_deg=(0, -20, 0), trans=(1.5, -0.55, -0.4), scale=(0.9,) * 3))
        b.add_proc("box", 0, _mirror(), T(rot_deg=(0, 15, 0), trans=(-0.1, -0.45, -1.5), scale=(1.1,) * 3))
        b.add_proc("geodesic", 1, H.material(emissive=(30, 27, 22), brdf=(0.3,) * 3), T(trans=(0.3, 1.7, 0.4), scale=(0.25,) * 3))
        if small_jade_last:
            one = np.float32([[-0.2, -0.99, 1.9], [0.9, -0.99, 2.1], [0.3, -0.2, 2.3]])
            b.add_mesh(one, np.int32([[0, 1, 2]]), _jade())
            two = np.float32([[-2.3, -0.99, 1.2], [-1.3, -0.99, 1.6], [-1.4, -0.1, 1.5], [-2.4, 0.0, 1.0]])
            b.add_mesh(two, np.int32([[0, 1, 2], [0, 2, 3]]), _jade())
        b.set_env_sky(16, 8)
        return b.build()
    finally:
        b.close()


def params(walk=_abi.WALK_REFERENCE):
    eye, cam = H.camera_orbit(5.0, 20.0, 30.0)
    return B.make_params(WIDTH, HEIGHT, SPP, eye, cam, threads=4, walk=walk)


def base():
    hs = _build()
    assert hs.n_triangles == 148 and len(hs.a["segs"]) == 6
    return hs


def _copy(hs):
    return HostScene({k: np.array(v, copy=True) for k, v in hs.a.items()}, hs.bvh_depth)


def _emissive(hs):
    return (hs.tri_f32()[:, 13:16] > np.float32(EMISSIVE_BAR)).any(1)


# ----------------------------------------------------------------------------------------------------------- the variants --

def patchwork(hs):
    """The five distinct material rows dealt round-robin over all triangles (obj_idx, geometry, norm kept): neighbours differ in
    material, an object has five; emit = the triangles now above the emissive bar."""
    tri = hs.a["triangles"]
    rows = np.unique(tri[:, MAT], axis=0)
    assert len(rows) == 5
    tri[:, MAT] = rows[np.arange(len(tri)) % 5]
    hs.a["emit"] = np.flatnonzero(_emissive(hs)).astype(np.int32)
    assert 25 <= len(hs.a["emit"]) <= 35


def thresholds(hs):
    """Emission of the non-light triangles cycled through the values around BOTH emissive tests (1.4e-5: bounce_classify,
    lean_can_shade, the emitter list's meaning; 1.5e-4: the mirror chain's `nonemissive`), in one channel, x, y and z in turn.  The
    triangles above the first bar end paths and are not in emit_indices."""
    tf = hs.tri_f32()
    idx = np.flatnonzero(~_emissive(hs))
    vals = np.float32([1.3e-5, 1.4e-5, 1.5e-5, 1.4e-4, 1.5e-4, 1.6e-4])
    for k, i in enumerate(idx):
        tf[i, 13 + (k // 6) % 3] = vals[k % 6]


def emit_odd(hs):
    """The list reversed, three entries twice, two triangles that do not emit."""
    e = hs.a["emit"][::-1]
    dark = np.flatnonzero(~_emissive(hs))[[7, 90]]
    hs.a["emit"] = np.concatenate([e, e[[0, 5, 11]], dark]).astype(np.int32)


def emit_none(hs):
    """No listed emitter, while the light stays emissive: light is found by hitting it only."""
    hs.a["emit"] = np.zeros(0, np.int32)


def _jade_ranges(hs):
    return [tuple(int(v) for v in hs.a["segs"][o]) for o in JADE_OBJECTS]


def prefix_reversed(hs):
    for b, e in _jade_ranges(hs):
        hs.a["prefix"][b:e + 1] = hs.a["prefix"][b:e + 1][::-1].copy()


def prefix_nan(hs):
    for b, e in _jade_ranges(hs):
        hs.a["prefix"][(b + e) // 2] = np.nan


def prefix_zero(hs):
    for b, e in _jade_ranges(hs):
        hs.a["prefix"][b:e + 1] = 0


def prefix_negated(hs):
    for b, e in _jade_ranges(hs):
        hs.a["prefix"][b:e + 1] *= -1


def prefix_inf(hs):
    """An object's TOTAL is inf: a factor of radiance, not only a search key (PathTrace.cu:1105, 1160).  Found with this variant on an
    MI355X: every counter equal, 699 NaN values in the module's frame against 633 in the oracle's (forward sum against unwound stack).
    include/jade_rt.h now has both backends refuse it (REFUSED below)."""
    for b, e in _jade_ranges(hs):
        hs.a["prefix"][e] = np.inf


def prefix_inf_inside(hs):
    """inf as a search key only, at the first midpoint of each jade object: u x A stays finite, the object is no longer monotone, and
    every search turns left there whatever u is (prefix-nan stops there instead)."""
    for b, e in _jade_ranges(hs):
        hs.a["prefix"][(b + e) // 2] = np.inf


def mapping_reversed(hs):
    """Exit triangles on other objects: a BSSRDF path leaves through a triangle whose refract_rate is not jade's."""
    hs.a["mapping"] = hs.a["mapping"][::-1].copy()


def mapping_constant(hs):
    hs.a["mapping"][:] = 3


def segs(hs):
    """Object 1's segment widened over object 2's (its prefix then restarts inside: not monotone), object 2 a single triangle: the
    reference's search returns mid = 0 for it, index_mapping[0] - a floor triangle."""
    s = hs.a["segs"]
    s[1, 1] = s[2, 1]
    s[2] = (s[2, 0] + 4, s[2, 0] + 4)


def obj_idx(hs):
    ti = hs.tri_i32()
    ti[:, 0] = (ti[:, 0] + 1) % 6


def normals(hs):
    """Every third normal flipped, every third scaled by 2.5: norm is read as given, never normalised or re-derived."""
    tf = hs.tri_f32()
    tf[0::3, 10:13] *= np.float32(-1)
    tf[1::3, 10:13] *= np.float32(2.5)


def small_jade_last(hs):
    """(not an edit: built with a 1-triangle and a 2-triangle jade object AFTER the others - mid = 0 away from the array's front)"""
    raise AssertionError("built, not edited")


VARIANTS = {
    "patchwork": patchwork, "thresholds": thresholds, "emit-odd": emit_odd, "emit-none": emit_none,
    "prefix-reversed": prefix_reversed, "prefix-nan": prefix_nan, "prefix-zero": prefix_zero, "prefix-negated": prefix_negated,
    "prefix-inf": prefix_inf, "prefix-inf-inside": prefix_inf_inside, "mapping-reversed": mapping_reversed, "mapping-constant": mapping_constant, "segs": segs,
    "obj_idx": obj_idx, "normals": normals, "small-jade-last": small_jade_last,
}
REFUSED = ("prefix-inf",)  # legal by range, refused by both backends with JADE_ERR_INVALID (include/jade_rt.h, jade_scene_desc)
RENDERED = tuple(sorted(set(VARIANTS) - set(REFUSED)))
SCHEDULED = ("patchwork", "thresholds", "small-jade-last")  # ... also rendered under every shading schedule and walk

_cache = {}


def scene(name):
    """The base scene ("base") or a variant, built once; callers do not edit what they get."""
    if name not in _cache:
        if name == "base":
            _cache[name] = base()
        elif name == "small-jade-last":
            hs = _build(small_jade_last=True)
            assert hs.n_triangles == 151 and [int(e - b + 1) for b, e in hs.a["segs"][6:]] == [1, 2] and hs.a["segs"][6, 0] == 148
            _cache[name] = hs
        else:
            hs = _copy(scene("base"))
            VARIANTS[name](hs)
            _cache[name] = hs
    return _cache[name]


_oracle_frames = {}


def oracle_frame(oracle, name):
    """(rgb, bgr, stats) of the scene through the oracle, rendered once per session."""
    if name not in _oracle_frames:
        with oracle.scene(scene(name)) as so:
            _oracle_frames[name] = so.render(params())
    return _oracle_frames[name]


def differing_pixels(a, b):
    """Share of the pixels whose radiance is not the same three floats (NaN = NaN)."""
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    return float((~same.all(-1)).mean())
