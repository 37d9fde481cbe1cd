"""tests/walk_ref.py held to the oracle, and what it says about the walks at depth ("the walks at depth").

No GPU: the model's node records and triangle tests are the oracle's ray by ray on every tree tests/test_gpu_deep_trees.py walks, so
the stack heights it reports for those rays are the heights the kernels' stacks reach on them - the evidence that the GPU tests
go through the spill area (level 8 and up of a lane's stack) at every level an accepted tree can fill, and that the depth gates
of prepare_scene (wide records, occluder cache) are sufficient bounds."""
import ctypes as C

import numpy as np
import pytest

from conftest import B, J, config_scene
from jaderaytracerendering_amd import _abi
import ray_helpers as RH

import walk_ref as W

FRAME_DEPTHS = (63, 64, 127)


def _col(res, key):
    return np.array([r[key] for r in res])


def _deferred(oracle, so, o, d, skip):
    """The oracle's own figure for rule a: entries waiting while the top one is followed, per ray (its histogram ends at 63)."""
    fn = oracle.lib.jade_oracle_stack_histogram
    fn.restype, fn.argtypes = None, [C.c_void_p, C.c_int]
    h = np.zeros(64, np.uint64)
    fn(h.ctypes.data, 1)
    out = np.zeros(len(o), np.int64)
    for i in range(len(o)):
        so.trace_rays(o[i:i + 1], d[i:i + 1], skip[i:i + 1])
        fn(h.ctypes.data, 1)
        assert h.sum() == 1
        out[i] = int(np.argmax(h))
    return out


def _scene_and_rays(name):
    if name in W.TREES:
        return W.deep_tree(name)
    if name.startswith("spine"):
        hs = W.spine_to_depth(config_scene("tinyjade")[0], int(name[5:]))
        rays = RH.rays(hs, 10, 11)
    else:
        hs = config_scene(name)[0]
        rays = RH.rays(hs, 42, 11)  # test_gpu_packet.py's batch
    return hs, rays, W.walk_batch(hs, *rays)


@pytest.mark.parametrize("name", W.TREES + tuple(f"spine{d}" for d in FRAME_DEPTHS) + ("tinyjade",))
def test_model_reads_what_the_oracle_reads(oracle, name):
    hs, (o, d, skip), res = _scene_and_rays(name)
    with oracle.scene(hs) as so:
        want = RH.oracle_per_ray(so, o, d, skip)
        deferred = _deferred(oracle, so, o, d, skip)
    assert np.array_equal(_col(res, "V"), want[3]), "node records per ray"
    assert np.array_equal(_col(res, "T"), want[4]), "triangle tests per ray"
    assert np.array_equal(np.minimum(_col(res, "ha"), 63), deferred), "deferred children per ray (rule a)"
    assert (want[0] >= 0).sum() > 50
    # the binary unit with a full FIFO every time is rule a again, and never more than one entry above the unit with room
    assert np.array_equal(_col(res, "hb_full"), _col(res, "ha"))
    assert ((_col(res, "hb") <= _col(res, "ha")) & (_col(res, "ha") <= _col(res, "hb") + 1)).all()
    # the wide walk meets the reference's leaves (rays without a NaN in the slab test: test_box_monotone.py)
    with np.errstate(divide="ignore"):
        finite = np.isfinite(o).all(1) & np.isfinite(np.float32(1) / d).all(1)
    for i in np.nonzero(finite)[0]:
        if "wide_leaves" in res[i]:
            assert sorted(res[i]["wide_leaves"]) == sorted(res[i]["leaves"]), i


def test_slab_is_the_monotone_tests_slab_where_no_nan_occurs():
    hs, (o, d, skip), _ = W.deep_tree("bushy82")
    T = W.Tree(hs)
    with np.errstate(divide="ignore"):
        finite = np.isfinite(np.float32(1) / d).all(1)
    assert finite.sum() > 300 and (~finite).sum() >= 40
    for i in np.nonzero(finite)[0]:
        assert np.array_equal(W.slab(T.aa, T.bb, o[i], d[i]), RH.slab(T.aa, T.bb, o[i], d[i]))


@pytest.mark.parametrize("D,height", [(9, 7), (10, 8), (11, 9), (12, 10), (63, 61), (64, 62), (82, 80), (83, 81), (124, 122), (125, 123),
                                      (127, 125)])
def test_comb_heights_are_reached(D, height):
    """Rule b on comb(D): D - 2 entries on the +z bundle.  Depths 9 .. 12 step through "all in LDS" (7), "exactly full" (8) and the
    first spilled levels (9, 10); depth 127 reaches 125 - the greatest height an accepted tree gives the binary unit - and 126 with the
    FIFO full (k_light), the oracle's own figure.  At least a wave's worth of rays sits at the maximum and another at height <= 1."""
    hs, (o, d, skip), res = W.deep_tree(f"comb{D}")
    hb, hf = _col(res, "hb"), _col(res, "hb_full")
    assert hs.bvh_depth == D and hb.max() == height and hf.max() == height + 1
    assert (hb[:64] == height).all(), "the +z bundle"
    assert (hb[64:128] <= 1).all(), "the -z bundle: a leaf first at every step"
    assert (hb == height).sum() >= 64 and (hb <= 1).sum() >= 64
    assert hf.max() + 1 <= W.STACK_CAPACITY - 1  # entries, the one being followed included
    if height > W.LDS_STACK:  # waves with lanes on both sides of the LDS levels: the spill branches run for some lanes only
        last = hb[384:448]    # the +z bundle, every fourth lane from a height of its own
        assert (last == height).sum() >= 40 and (last <= W.LDS_STACK).sum() >= 4
    if height > 2 * W.LDS_STACK:
        mixed = hb[128:192]   # origins spread along the comb, up and down
        assert (mixed <= W.LDS_STACK - 3).sum() >= 4 and (mixed > W.LDS_STACK).sum() >= 4 and len(set(mixed.tolist())) >= 16
    # every spill level up to the maximum is written by some ray (a ray at height h went through all the levels below h)
    assert _col(res, "V").max() == 2 * D - 1 and _col(res, "T")[:64].min() == D


def test_the_gates_are_sufficient_bounds():
    """prepare_scene: wide records where 3 * ((depth + 1) / 2) + 1 + 3 <= 128, an occluder cache where depth + 3 <= 127.  Over every
    tree and batch: the wide walk's height, with the three entries a cached start puts under it, is within 3 * ((depth + 1) / 2) + 4
    - which is <= 128 wherever the gate lets wide records be built; the binary unit's (FIFO full) with those three within 127
    wherever the gate allows the cache.  The thresholds: 82 / 83 and 124 / 125."""
    assert W.wide_fits(82) and not W.wide_fits(83) and W.cache_fits(124) and not W.cache_fits(125)
    for name in W.TREES + tuple(f"spine{d}" for d in FRAME_DEPTHS):
        hs, _, res = _scene_and_rays(name)
        depth = hs.bvh_depth
        assert _col(res, "hb_full").max() + 1 <= W.STACK_CAPACITY, name  # the oracle's stack[128]
        if W.cache_fits(depth):
            assert _col(res, "hb_full").max() + W.WIDE_CACHED_EXTRA <= W.STACK_CAPACITY - 1, name
        if "hc" in res[0]:
            hc = _col(res, "hc").max() + W.WIDE_CACHED_EXTRA
            assert hc <= 3 * ((depth + 1) // 2) + 4, name
            assert not W.wide_fits(depth) or hc <= W.STACK_CAPACITY, name


def test_wide_height_and_slack_at_the_gate():
    """bushy_comb(82), the deepest tree that gets wide records, on the +z bundle: 40 units of three pushes and one of one = 121
    entries from the root, 124 behind a cached start - 4 short of the 128 the stack holds (the gate's bound: 127).  bushy_comb(83)
    would reach 125 and gets no wide records."""
    for D, want in ((82, 121), (83, 122)):
        hs, _, res = W.deep_tree(f"bushy{D}")
        hc = _col(res, "hc")
        assert hc.max() == want and (hc[:64] == want).all() and (hc == want).sum() >= 64
        assert want + W.WIDE_CACHED_EXTRA <= 3 * ((D + 1) // 2) + 4
    assert W.STACK_CAPACITY - (121 + W.WIDE_CACHED_EXTRA) == 4
    # the binary walks on the same trees: two entries for two levels
    assert _col(W.deep_tree("bushy82")[2], "hb").max() == 80


def test_heights_of_the_suite_before_the_deep_trees():
    """For the record: what tests/test_gpu_packet.py's rays - the deepest walks of the suite until the deep trees -
    reach on C2 (20 levels): 9 entries, one level of the spill area; on tiny / tinyjade nothing leaves LDS."""
    got = {}
    for name, packets in (("tiny", 42), ("tinyjade", 42), ("C2", 24)):
        hs, _ = config_scene(name)
        res = W.walk_batch(hs, *RH.rays(hs, packets, 11))
        got[name] = tuple(int(_col(res, k).max()) for k in ("ha", "hb", "hc"))
    assert got == {"tiny": (6, 5, 8), "tinyjade": (8, 7, 8), "C2": (9, 9, 10)}, got


@pytest.mark.parametrize("depth", FRAME_DEPTHS)
def test_frames_over_a_spine_reach_the_spill_area(depth):
    """spine_to_depth(tinyjade, depth): the camera rays of the 48 x 40 frame test_gpu_deep_trees.py renders (pixel corners: close
    enough to the jittered rays) - a wave's worth of them keeps more than the LDS levels, under the binary rule."""
    hs0, cfg = config_scene("tinyjade")
    hs = W.spine_to_depth(hs0, depth)
    assert hs.bvh_depth == depth and np.array_equal(hs.a["triangles"], hs0.a["triangles"]) and np.array_equal(hs.a["emit"], hs0.a["emit"])
    w, h = 48, 40
    M = np.asarray(list(cfg.camera), np.float64).reshape(4, 4)
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    v = np.stack([(-1 + 2.0 / w * x) * (w / h), -1 + 2.0 / h * y, np.full(x.shape, -1.5)], -1).reshape(-1, 3)
    d = (v @ M[:3, :3]).astype(np.float32)  # dir[r] = sum_c M[c][r] v[c]
    o = np.broadcast_to(np.float32(list(cfg.eye)), d.shape).copy()
    res = W.walk_batch(hs, o, d, np.full(len(o), -1))
    hb = _col(res, "hb")
    assert (hb > W.LDS_STACK).sum() >= 20 and hb.max() >= 18, (int((hb > W.LDS_STACK).sum()), int(hb.max()))


@pytest.mark.parametrize("which", ["oracle", "hip"])
def test_depth_127_is_accepted_and_128_refused(which, oracle):
    """validate_desc of both backends: JADE_BVH_STACK_CAPACITY - 1 levels.  (The HIP module validates before it looks for a device: on a
    machine without one the accepted tree gets as far as JADE_ERR_DEVICE.)"""
    be = oracle if which == "oracle" else J.hip()
    try:
        be.scene(W.deep_tree("comb127")[0]).close()
    except B.JadeError as e:
        assert which == "hip" and e.code == _abi.JADE_ERR_DEVICE
    with pytest.raises(B.JadeError) as ei:
        be.scene(W.comb(128))
    assert ei.value.code == _abi.JADE_ERR_UNSUPPORTED and str(ei.value)
