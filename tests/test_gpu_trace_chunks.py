"""Claims larger than 64 rays ("k_trace"): a wave of k_trace takes `chunk` queue positions per atomic and refills its idle lanes
out of that claim.  trace_chunk_for leaves the chunk at 64 until a launch has 16 x waves x 64 rays - millions on a full grid - so no small
queue ever ran: a wave that takes several refills out of one claim (take < avail, lbase advancing inside [lbase, lend)), a claim clipped
by the queue's length, waves left with nothing because a few claimed everything.  JADE_TRACE_CHUNK_RAYS (a test hook) names the chunk, for
host-followed launches and - in place of the device's own copy of the rule - for batched ones.

Raw rays (jade_trace_rays) against the oracle ray by ray, at ray counts around every chunk; frames against the chunk-64 render bit for bit
and counter for counter (the reference walk: every count is a function of the rays alone), one of them against the oracle."""
import numpy as np
import pytest

import queue_hooks as Q
from conftest import config_scene
import ray_helpers as RH
from render_helpers import TOL, assert_parity

pytestmark = pytest.mark.gpu

CHUNKS = (64, 128, 256, 512)
INF = np.float32(2147483647.0)  # JADE_INF_F, the walk's own infinity ("any recorded hit", jade_device.h) - the largest limit the integrator can ask for.
# (An IEEE infinity is not a limit the integrator can produce - shadow_limit returns a distance or JADE_INF_F - and the walk is not defined for
# it: its best distance starts at JADE_INF_F, already below such a limit.)


def _counts(chunk):
    return sorted({1, 63, 64, 65, chunk - 1, chunk, chunk + 1, 3 * chunk + 17})


N_MAX = 3 * 512 + 17


def _chunk(c):
    return {"JADE_TRACE_CHUNK_RAYS": str(c)}


# -------------------------------------------------------------------------------------------------------------------- raw rays --

_want = {}


def _oracle_rays(oracle, name):
    """The rays of tests/test_gpu_packet.py (coherent and incoherent packets, rays leaving triangles, zero components) and the oracle's
    answer for each, its own node records and triangle tests included: once per scene."""
    if name not in _want:
        hs, _ = config_scene(name)
        o, d, skip = RH.rays(hs, (N_MAX + 63) // 64, 11)
        with oracle.scene(hs) as so:
            _want[name] = (o, d, skip) + RH.oracle_per_ray(so, o, d, skip)
    return _want[name]


def _assert_rays(got, want, n, what):
    idx, dist, pt, st = got
    w_idx, w_dist, w_pt, w_v, w_t = (a[:n] for a in want)
    assert np.array_equal(idx, w_idx), what
    assert np.array_equal(dist.view(np.uint32), w_dist.view(np.uint32)), what  # (a miss keeps INF on both sides)
    hit = w_idx >= 0
    assert np.array_equal(pt[hit].view(np.uint32), w_pt[hit].view(np.uint32)), what
    assert (st.nodes_visited, st.tris_tested) == (int(w_v.sum()), int(w_t.sum())), what


@pytest.mark.parametrize("name", ["tiny", "C2"])
def test_raw_rays_at_every_chunk_match_the_oracle_ray_by_ray(oracle, hip_debug, name):
    o, d, skip, *want = _oracle_rays(oracle, name)
    hs, _ = config_scene(name)
    assert (want[0] >= 0).sum() > 200 and (want[0] < 0).sum() > 200
    inf_limits = np.full(N_MAX, INF, np.float32)
    base = {}  # the chunk-64 answers under a limit of INF, for every ray count of every chunk
    with Q.environment(_chunk(64)), hip_debug.scene(hs) as sc:
        for n in sorted({n for chunk in CHUNKS for n in _counts(chunk)}):
            base[n] = RH.trace_limit(hip_debug, sc, o[:n], d[:n], skip[:n], inf_limits[:n])
    for chunk in CHUNKS:
        with Q.environment(_chunk(chunk)), hip_debug.scene(hs) as sc:
            for n in _counts(chunk):
                what = (name, chunk, n)
                _assert_rays(sc.trace_rays(o[:n], d[:n], skip[:n]), want, n, what)
                # ... and through jade_debug_trace_rays_limit.  A NaN limit never ends a walk: the reference's answer and work, again.
                nan = np.full(n, np.nan, np.float32)
                _assert_rays(RH.trace_limit(hip_debug, sc, o[:n], d[:n], skip[:n], nan), want, n, what + ("NaN limits",))
                # A limit of INF ends a walk at ANY recorded hit - which one depends on the other rays of the wave (jade_hip.hip,
                # jade_debug_trace_rays_limit), and so on the chunk.  What does not: the same rays miss, with the same bits; a ray that hits
                # reports a triangle at a distance not nearer than its nearest hit; and wherever the triangle is the chunk-64 run's, so
                # are distance and point.
                i1, t1, p1, _ = RH.trace_limit(hip_debug, sc, o[:n], d[:n], skip[:n], inf_limits[:n])
                i0, t0, p0, _ = base[n]
                miss = want[0][:n] < 0
                assert np.array_equal(i1 < 0, miss) and np.array_equal(i0 < 0, miss), what
                assert np.array_equal(t1[miss].view(np.uint32), want[1][:n][miss].view(np.uint32)), what
                assert (t1[~miss] >= want[1][:n][~miss]).all() and (t1[~miss] < INF).all(), what
                same = (i1 == i0) & ~miss
                assert np.array_equal(t1[same].view(np.uint32), t0[same].view(np.uint32)), what
                assert np.array_equal(p1[same].view(np.uint32), p0[same].view(np.uint32)), what


def test_an_ignored_chunk_is_the_rule(oracle, hip_debug):
    """Not a multiple of 64, or outside 64..512: the launch is the default one (the CPU file holds the rule; here it reaches a kernel)."""
    o, d, skip, *want = _oracle_rays(oracle, "tiny")
    hs, _ = config_scene("tiny")
    for bad in ("0", "100", "576", "-64"):
        with Q.environment(_chunk(bad)), hip_debug.scene(hs) as sc:
            _assert_rays(sc.trace_rays(o, d, skip), want, len(o), bad)


# ---------------------------------------------------------------------------------------------------------------------- frames --

TAIL0 = {"JADE_TAIL": "0"}  # (with k_tail this frame is one k_trace launch: without it, ~190, most of them batched)


@pytest.fixture(scope="module")
def chunk64(hip_debug):
    return Q.render(hip_debug, "tinyjade", {**TAIL0, **_chunk(64)})


def test_the_chunk_64_frame_is_the_oracles(oracle, hip_debug, chunk64):
    hs, p, _ = Q.frame("tinyjade")
    with oracle.scene(hs) as so:
        want = so.render(p)
    err = assert_parity(want, chunk64[:3], TOL)
    print(f"tinyjade, chunk 64, against the oracle: relative L2 {err:.3g}")
    big = Q.render(hip_debug, "tinyjade", {**TAIL0, **_chunk(512)})
    assert_parity(want, big[:3], TOL)


@pytest.mark.parametrize("chunk", CHUNKS)
def test_frames_at_every_chunk_are_the_chunk_64_frame(hip_debug, chunk64, chunk):
    for batch in ("0", "1"):
        for per_cu in ("1", None):
            env = {**TAIL0, **_chunk(chunk), "JADE_BATCH": batch}
            if per_cu:
                env["JADE_TRACE_BLOCKS_PER_CU"] = per_cu
            out = Q.render(hip_debug, "tinyjade", env)
            Q.assert_same_frame(out, chunk64, env)
            assert out[2].tail_launches == 0 and out[3] == chunk64[3]
            if batch == "1" and chunk > 64:
                assert out[2].trace_launches > 96, "passes ran in batches: the device took the host's chunk"
    # ... and with k_tail, the fused first pass' hand-over as the one queue; unfused, the camera rays' 6144
    for env in ({}, {"JADE_FUSED": "0"}, {"JADE_FUSED": "0", "JADE_SHADE_SPLIT": "0", **TAIL0}):
        Q.assert_same_frame(Q.render(hip_debug, "tinyjade", {**env, **_chunk(chunk)}), chunk64, (env, chunk))


def test_chunk_512_across_the_record_boundary_and_in_an_ordered_queue(hip_debug, chunk64):
    big = _chunk(512)
    out = Q.render(hip_debug, "tinyjade", {**TAIL0, **big, "JADE_RAYQ_CAP": "100"})
    Q.assert_same_frame(out, chunk64, "chunk 512, cap 100")
    assert out[3][0] > 0 and out[3][1] > 0
    sort = {"JADE_SORT": "1", "JADE_SORT_MIN": "64"}
    out = Q.render(hip_debug, "tinyjade", {**TAIL0, **big, **sort})
    Q.assert_same_frame(out, chunk64, "chunk 512, ordered")
    out = Q.render(hip_debug, "tinyjade", {**TAIL0, **big, **sort, "JADE_RAYQ_CAP": "100"})
    Q.assert_same_frame(out, chunk64, "chunk 512, ordered, cap 100")
    assert out[3][0] > 0 and out[3][1] > 0
    # C2's frame (ordered by its own setting): the statue's deep walks, chunk 512 against chunk 64
    ref = Q.render(hip_debug, "C2", _chunk(64))
    for env in ({}, {"JADE_RAYQ_CAP": "100"}, TAIL0):
        Q.assert_same_frame(Q.render(hip_debug, "C2", {**env, **big}), ref, ("C2", env))
