"""The walks on the deepest trees the module accepts ("the walks at depth").

Every traversal kernel keeps JADE_LDS_STACK = 8 stack levels per lane in LDS and spills the deeper ones to a global area; a caller's
BVH may have 127 levels; three gates by depth decide which walks a scene gets (the packet form up to 63, wide records up to 82, the
occluder cache up to 124).  Here: combs of 9 .. 127 levels (tests/walk_ref.py), on which tests/test_walk_ref_cpu.py has shown that
the rays below fill a lane's stack to depth - 2 entries beside lanes that stay in LDS, and that a wide unit's three pushes reach 121 -
walked by every form of the walk and compared with the oracle bit for bit; the gates at their thresholds; the grids of every kernel
that is handed the spill area; and frames of tinyjade under a spine of 63, 64 and 127 levels."""
import ctypes as C

import numpy as np
import pytest

from conftest import (B, assert_cached_walk_equals_reference_walk, assert_early_exit_equals_reference_walk, config_scene, counters,
                      rel_l2)
from jaderaytracerendering_amd import _abi

import ray_helpers as RH
import walk_ref as W

pytestmark = pytest.mark.gpu

_want = {}


def _reference(oracle, name):
    """The oracle's answer, node records and triangle tests for every ray of a tree's batch, and its answers for the batch of
    queries that leave triangles: computed once."""
    if name not in _want:
        hs, (o, d, skip), _ = W.deep_tree(name)
        with oracle.scene(hs) as so:
            _want[name] = RH.oracle_per_ray(so, o, d, skip), so.trace_rays(*_source_rays(hs))[:3]
    return _want[name]


def _source_rays(hs):
    """256 rays along z (a little tilted), every one from one of (up to) 16 triangles, which it skips: the keys of the occluder cache repeat."""
    rng = np.random.default_rng(17)
    v = hs.vertices()
    src = rng.choice(len(v), min(16, len(v)), replace=False)[rng.integers(0, min(16, len(v)), 256)].astype(np.int32)
    o = np.ascontiguousarray(v[src].mean(1), np.float32)
    d = np.zeros((256, 3), np.float32)
    d[:, :2] = rng.uniform(2e-4, 1e-3, (256, 2)) * rng.choice([-1.0, 1.0], (256, 2))
    d[:, 2] = rng.choice([-1.0, 1.0], 256)
    return o, d, src


def _grids(hip, sc):
    fn = hip.lib.jade_debug_scene_grids  # libjade_hip_debug.so only (not part of jade_rt.h)
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
    out = np.zeros(4, np.int32)
    hip.check(fn(sc._h, out.ctypes.data))
    return [int(x) for x in out]  # trace_blocks, trace_blocks_wide, light_blocks, packet_blocks


@pytest.mark.parametrize("name,wide", [(n, w) for n in W.TREES for w in ("0", "1")])  # shallow to deep
def test_raw_rays_are_the_oracles_at_every_depth(oracle, hip_debug, name, wide, monkeypatch):
    """A tree's batch (walk_ref.comb_rays: the greatest height, a leaf at every step, every height in one wave, rays that leave
    half-way, rays that skip their triangle, the NaN-faithful unit) through jade_trace_rays, through the packet form where the tree
    is not too deep for it, through k_trace with limits (JADE_WIDE=1: wide units where the tree has wide records) and three times
    through the occluder cache of one handle."""
    hip = hip_debug
    monkeypatch.setenv("JADE_WIDE", wide)
    hs, (o, d, skip), _ = W.deep_tree(name)
    want, want_src = _reference(oracle, name)
    n = len(o)
    rng = np.random.default_rng(3)
    with hip.scene(hs) as sh:
        # ---- the reference's walk: binary units, every leaf met
        got = sh.trace_rays(o, d, skip)
        RH.same_answers(got, want)
        assert got[3].nodes_visited == int(want[3].sum()) and got[3].tris_tested == int(want[4].sum())
        hitm = want[0] >= 0
        assert hitm.sum() >= 300 and (~hitm).sum() >= 10
        # ---- the packet form: one scalar stack of JADE_PACKET_MAX_DEPTH + 1 entries per wave
        if hs.bvh_depth <= W.PACKET_MAX_DEPTH:
            pk = RH.packet_rays(hip, sh, o, d, skip)
            assert not (pk[0] == -3).any(), "no two leaves tie on these trees: no packet is given up"
            RH.same_answers(pk, want)
            assert np.array_equal(pk[3].astype(np.int64), want[3]), "node records per ray"
            assert np.array_equal(pk[4].astype(np.int64), want[4]), "triangle tests per ray"
        else:
            with pytest.raises(B.JadeError) as ei:
                RH.packet_rays(hip, sh, o, d, skip)
            assert ei.value.code == _abi.JADE_ERR_UNSUPPORTED
        # ---- k_trace / k_trace_wide with a limit per ray: all NaN (the whole walk, whatever its units), all INF, a mixture
        nan = RH.trace_limit(hip, sh, o, d, skip, RH.nan_limit(n))
        RH.same_answers(nan, want)
        assert nan[3].tris_tested == int(want[4].sum())  # (no tie on these trees: no ray is walked twice)
        if not RH.flags(hip, sh) & 2:
            assert nan[3].nodes_visited == int(want[3].sum())
        for limit in (np.full(n, RH.INF), RH.limits(rng, hitm, want[1])):
            got = RH.trace_limit(hip, sh, o, d, skip, limit)
            ends = RH.assert_answers(got, want, limit, skip)
            assert ends.sum() >= 100
            assert got[3].tris_tested < int(want[4].sum())
        # ---- the occluder cache: queries that leave triangles, three times on this handle
        so_, sd_, ssrc = _source_rays(hs)
        limit = RH.limits(rng, want_src[0] >= 0, want_src[1])
        answered = []
        for rnd in range(3):
            got = RH.trace_limit(hip, sh, so_, sd_, ssrc, limit, cached=True)
            ends = RH.assert_answers(got, want_src, limit, ssrc)
            answered.append(int(got[3].rays_cached))
            assert answered[-1] <= ends.sum()  # the cache only ever answers "yes" queries
        assert ends.sum() >= 60
        if RH.flags(hip, sh) & 4:
            assert answered[0] <= answered[-1] and answered[-1] > 0, answered  # warm rounds start from what the cold one learnt
        else:
            assert answered == [0, 0, 0]


def test_gates_at_their_thresholds(hip_debug, monkeypatch):
    """jade_debug_scene_flags - 1: boxes nested, 2: wide records, 4: occluder cache - and jade_debug_scene_grids with JADE_WIDE=1."""
    hip = hip_debug
    monkeypatch.setenv("JADE_WIDE", "1")
    want = {"comb63": 7, "comb64": 7, "comb82": 7, "comb83": 5, "bushy82": 7, "bushy83": 5, "comb124": 5, "comb125": 1, "comb127": 1,
            "comb100m5": 1}  # (a missing child: the general walk - neither wide records nor a cache)
    for name in W.TREES:
        hs = W.deep_tree(name)[0]
        with hip.scene(hs) as sh:
            flags, g = RH.flags(hip, sh), _grids(hip, sh)
        assert flags & 1, name
        assert flags == want.get(name, 7), name
        assert (g[3] > 0) == (hs.bvh_depth <= W.PACKET_MAX_DEPTH), (name, g)
        assert g[0] > 0 and 0 < g[1] <= g[0] and 0 < g[2] <= g[0], (name, g)


@pytest.mark.parametrize("per_cu", ["", "1", "2"])
def test_grids_stay_within_the_spill_area(hip_debug, per_cu, monkeypatch):
    """The stack spill area holds 120 levels for trace_blocks x JADE_TRACE_BLOCK threads (setup_state): thread gtid of a grid of G
    threads writes level k at (k - 8) * G + gtid, so every kernel that is handed the area - k_trace_wide, k_light, k_tail (whose list is
    clamped to the same figure), the guide pass - must be launched with at most that many, whatever the occupancy sweep's setting."""
    hip = hip_debug
    monkeypatch.setenv("JADE_WIDE", "1")
    if per_cu:
        monkeypatch.setenv("JADE_TRACE_BLOCKS_PER_CU", per_cu)
    grids = []
    for hs in (W.deep_tree("comb63")[0], W.deep_tree("comb127")[0], config_scene("tinyjade")[0]):
        with hip.scene(hs) as sh:
            grids.append(_grids(hip, sh))
    for g in grids:
        assert g[0] > 0 and 0 < g[1] <= g[0] and 0 < g[2] <= g[0], g
    assert grids[0][3] > 0 and grids[1][3] == 0 and grids[2][3] > 0
    assert grids[0][:3] == grids[1][:3] == grids[2][:3]  # (the grids follow the kernels' occupancy, not the scene)


def test_depth_127_is_accepted_and_128_refused(hip):
    with hip.scene(W.deep_tree("comb127")[0]) as sh:
        i, t, p, st = sh.trace_rays(np.float32([[0, -0.2, -1]]), np.float32([[1e-4, 1e-4, 1]]), np.int32([-1]))
    assert i[0] >= 0 and st.nodes_visited == 2 * 127 - 1 and st.tris_tested == 127
    with pytest.raises(B.JadeError) as ei:
        hip.scene(W.comb(128))
    assert ei.value.code == _abi.JADE_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------------------ frames --

_frames = {}


def _spine_frame(oracle, depth):
    """tinyjade under a spine (walk_ref.spine_to_depth), its 48 x 40 frame at 4 spp, and the oracle's render of it: made once."""
    if depth not in _frames:
        hs0, cfg = config_scene("tinyjade")
        hs = W.spine_to_depth(hs0, depth)
        p = B.params_from_config(cfg, spp=4)
        p.width, p.height = 48, 40
        with oracle.scene(hs) as so:
            _frames[depth] = hs, p, so.render(p)
    return _frames[depth]


@pytest.mark.parametrize("depth,wide", [(dp, w) for dp in (63, 64, 127) for w in ("0", "1")])
def test_frames_over_a_spine(oracle, hip_debug, depth, wide, monkeypatch):
    """The whole integrator on a deep tree: the first pass is k_light_packet at 63 levels and k_light at 64 and 127, the wavefront
    passes and k_tail keep up to twenty-odd entries per lane (test_walk_ref_cpu.py).  The project's parity bar against the oracle
    - every counter equal, relative L2 <= 1e-4 - and the three walks the same bits."""
    hip = hip_debug
    monkeypatch.setenv("JADE_WIDE", wide)
    hs, p, (r_o, b_o, st_o) = _spine_frame(oracle, depth)
    q = type(p).from_buffer_copy(p)
    q.walk = _abi.WALK_EARLY_EXIT
    with hip.scene(hs) as sh:
        flags, g = RH.flags(hip, sh), _grids(hip, sh)
        ref = sh.render(p)
        early = sh.render(q)
        assert_cached_walk_equals_reference_walk(sh, p, ref)
    assert flags == (7 if wide == "1" and depth <= 82 else 5 if depth <= 124 else 1)
    assert (g[3] > 0) == (depth <= W.PACKET_MAX_DEPTH)
    assert counters(ref[2]) == counters(st_o)
    assert np.array_equal(np.isnan(ref[0]), np.isnan(r_o))
    assert rel_l2(ref[0], r_o) <= 1e-4
    assert_early_exit_equals_reference_walk(ref, early, fewer=not flags & 2)  # (a wide unit counts grandchildren, and a tie is walked twice)


def test_guides_over_the_deepest_spine_match_the_spec(hip):
    """jade_render_guides at 127 levels against jade_spec's float64 camera ray and brute-force hit, as
    test_gpu_denoise.py::test_guides_match_the_spec does - on the pixels whose camera ray keeps more entries than the LDS levels
    hold (walk_ref's rule b on the very ray the spec draws: the guide pass goes through the spill area for them) and on as many
    others.  The float64 brute force costs 50 ms a pixel, hence a choice of 64 pixels of the 48 x 40."""
    import jade_spec
    from guide_cases import Geometry, spec_guide
    hs0, cfg = config_scene("tinyjade")
    hs = W.spine_to_depth(hs0, 127)
    w, h = 48, 40
    p = B.params_from_config(cfg, spp=4)
    p.width, p.height = w, h
    M = np.asarray(list(p.camera), np.float64).reshape(4, 4)
    T, eye = W.Tree(hs), np.float32(list(p.eye))
    height = {}
    for y in range(h):
        for x in range(w):
            rng = jade_spec.wang_stream(x, y, p.frame)
            lx = (-1 + 2.0 / w * (x + next(rng) - 0.5)) * (w / h)
            ly = -1 + 2.0 / h * (y + next(rng) - 0.5)
            height[x, y] = W.walk(T, eye, (np.array([lx, ly, -1.5]) @ M[:3, :3]).astype(np.float32))["hb"]
    deep = sorted((k for k in height if height[k] > W.LDS_STACK), key=lambda k: (-height[k], k))[:32]
    assert len(deep) == 32 and height[deep[0]] >= 16
    rest = [k for k in sorted(height) if k not in deep][::(w * h - 32) // 32][:32]
    with hip.scene(hs) as sc:
        sc.begin(p)
        sc.step(4)
        g = sc.guides(1)
    S = Geometry(hs)
    ok = 0
    for x, y in deep + rest:
        a, n, z = spec_guide(S, x, y, p, p.frame)
        good = (np.allclose(g["albedo"][y, x], a, rtol=0, atol=1e-6) and np.allclose(g["normal"][y, x], n, rtol=0, atol=1e-6)
                and abs(g["depth"][y, x] - z) <= 1e-5 * max(1.0, abs(z)))
        ok += bool(good)
    assert ok >= 0.99 * 64, f"{ok} of 64 pixels agree with the spec"
