"""Caller-shaped trees on the device ("caller-shaped trees"): tests/tree_shapes.py's list - unused nodes behind the tree,
renumbered trees, nodes with two parents, overlapping and missing leaves, degenerate roots, dishonest boxes - through every form of
the walk and through the integrator, against the oracle.

The shapes are the ones tests/test_scene_prep_cpu.py has held against the statement of the records on the host (every reference
inside its array); what is new here is the kernels reading those records: jade_trace_rays, k_trace with limits (binary and wide
units), the packet form, the occluder cache, and a small frame under three shading schedules and the three walks."""
import numpy as np
import pytest

from conftest import (B, assert_cached_walk_equals_reference_walk, assert_early_exit_equals_reference_walk, config_scene, counters,
                      rel_l2)
from jaderaytracerendering_amd import _abi
import ray_helpers as RH

import prep_ref as P
import scene_shapes as SS
import tree_shapes as TS

pytestmark = pytest.mark.gpu

TOL = 1e-4  # relative L2 on pre-tonemap radiance (BASELINE.json north_star)
FRAME_SCHEDULES = (0, 1, 4)  # of scene_shapes.SCHEDULES: packets + binned shading; k_light + wide units + no k_tail; the unfused first pass + wide units


def _expected_flags(hip, hs, wide):
    """jade_debug_scene_flags from the facts prepare_scene reports on the host: 1 boxes nested, 2 wide records, 4 occluder cache."""
    rc, p = P.prepare(hip.lib, hs, wide)
    assert rc == 0
    general = bool(p.missing_child) or not p.nested
    cache = not general and bool(p.cache_fits) and p.n_internal > 1
    return (1 if p.nested else 0) | (2 if len(p.nodes4) else 0) | (4 if cache else 0), general, p


@pytest.mark.parametrize("name,wide", [(n, w) for n in TS.ACCEPTED for w in ("0", "1")])
def test_raw_rays_are_the_oracles_on_every_shape(oracle, hip_debug, name, wide, monkeypatch):
    """The shape's 4096 rays through jade_trace_rays (triangle, distance bits, hit-point bits, node records and triangle tests),
    through the packet form (per ray, wherever the packet was not given up for a tie), through k_trace with a limit per ray and three
    times through the occluder cache of one handle."""
    hip = hip_debug
    monkeypatch.setenv("JADE_WIDE", wide)
    sh, hs = TS.BY_NAME[name], TS.scene(name)
    o, d, skip = TS.rays(name)
    want = P.reference(oracle, name)
    n = len(o)
    rng = np.random.default_rng(3)
    flags_want, general, p = _expected_flags(hip, hs, int(wide))
    with hip.scene(hs) as sc:
        flags = RH.flags(hip, sc)
        assert flags == flags_want, (flags, flags_want)
        if p.n_internal > 1:
            assert (flags & 6 == 0) == general, "neither wide records nor a cache exactly where the walk is the general one"
        if sh.same_as_base:
            with hip.scene(TS.base_scene(sh.base)) as sb:
                assert flags == RH.flags(hip, sb)
        # ---- the reference's walk
        got = sc.trace_rays(o, d, skip)
        RH.same_answers(got, want)
        assert got[3].nodes_visited == int(want[3].sum()) and got[3].tris_tested == int(want[4].sum())
        hitm = want[0] >= 0
        # ---- the packet form
        pk = RH.packet_rays(hip, sc, o, d, skip)
        given_up = pk[0] == -3
        # (a packet in which two leaves tie for some ray's best distance is given up, test_gpu_packet.py: a triangle in two leaves, and in
        # the 148-triangle base the boxes that stand ON the floor - a ray through a contact face)
        assert (~given_up).sum() >= (64 if sh.group == "cover" else n // 2), int(given_up.sum())  # (packets 0-31 go anywhere: no contact face in most)
        assert (given_up.reshape(-1, 64).all(1) == given_up.reshape(-1, 64).any(1)).all(), "a packet is given up as a whole"
        RH.same_answers(pk, want, ~given_up)
        assert np.array_equal(pk[3].astype(np.int64)[~given_up], want[3][~given_up]), "node records per ray"
        assert np.array_equal(pk[4].astype(np.int64)[~given_up], want[4][~given_up]), "triangle tests per ray"
        # ---- k_trace / k_trace_wide with a limit per ray: none (the whole walk), any hit, a mixture
        RH.same_answers(RH.trace_limit(hip, sc, o, d, skip, RH.nan_limit(n)), want)
        ends = RH.assert_answers(RH.trace_limit(hip, sc, o, d, skip, np.full(n, RH.INF)), want, np.full(n, RH.INF), skip)
        assert sh.empty or ends.sum() >= 100  # (every ray the oracle finds a hit for)
        limit = RH.limits(rng, hitm, want[1])
        ends = RH.assert_answers(RH.trace_limit(hip, sc, o, d, skip, limit), want, limit, skip)
        assert sh.empty or ends.any()
        # ---- the occluder cache: the rays that leave triangles are its queries; three rounds on this handle
        limit = RH.limits(rng, hitm, want[1])
        answered = []
        for _ in range(3):
            got = RH.trace_limit(hip, sc, o, d, skip, limit, cached=True)
            ends = RH.assert_answers(got, want, limit, skip)
            answered.append(int(got[3].rays_cached))
            assert answered[-1] <= ends.sum()
        if not flags & 4:
            assert answered == [0, 0, 0]


_frames = {}


def _frame(oracle, name):
    """The shape's scene, its 48 x 48 frame at 4 spp from the base's camera, and the oracle's render of it: made once."""
    if name not in _frames:
        sh, hs = TS.BY_NAME[name], TS.scene(name)
        p = SS.params() if sh.base == "base" else B.params_from_config(config_scene(sh.base)[1], spp=4)
        p.width, p.height, p.spp = 48, 48, 4
        with oracle.scene(hs) as so:
            _frames[name] = hs, p, so.render(p)
    return _frames[name]


@pytest.mark.parametrize("name", TS.ACCEPTED)
def test_frames_meet_the_parity_bar_under_three_schedules_and_walks(oracle, hip, name, monkeypatch):
    """Every work counter the oracle's, NaN at the same places, the radiance within 1e-4 relative L2, the bytes within one code; the
    early-exit and the cached walk the same bits as the reference walk; the three schedules the same bits."""
    hs, p, (r_o, b_o, st_o) = _frame(oracle, name)
    q = type(p).from_buffer_copy(p)
    q.walk = _abi.WALK_EARLY_EXIT
    first = None
    for k in FRAME_SCHEDULES:
        SS.set_schedule(monkeypatch, SS.SCHEDULES[k])
        with hip.scene(hs) as sc:
            ref = sc.render(p)
            early = sc.render(q)
            assert_cached_walk_equals_reference_walk(sc, p, ref)
        assert_early_exit_equals_reference_walk(ref, early, fewer=False)  # (ties - a triangle in two leaves - are walked twice)
        if first is None:
            first = ref
            assert counters(ref[2]) == counters(st_o)
            assert np.array_equal(np.isnan(ref[0]), np.isnan(r_o))
            fin = np.isfinite(r_o)
            assert rel_l2(ref[0][fin], r_o[fin]) <= TOL
            assert np.abs(ref[1].astype(np.int16) - b_o.astype(np.int16)).max() <= 1
        else:
            assert np.array_equal(ref[0].view(np.uint32), first[0].view(np.uint32)) and np.array_equal(ref[1], first[1]), k
            assert counters(ref[2]) == counters(first[2]), k
