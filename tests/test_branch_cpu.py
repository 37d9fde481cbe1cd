"""JADE_BRANCH_STRATIFIED without a GPU (include/jade_bvh.h, "The branch draws, stated"; tests/branch_spec.py is that text in numpy): the
host build of branch_number against the statement bit for bit, the net property of the two sequences under random shifts, the shares
a pixel's samples take, the shift's uniformity over pixels, shade_mode_for's twelve new modes and their refusals, the tables the device
tests take from the statement alone, and mode_seams' checks on the mode's case against a stand-in that can be made wrong."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import branch_cases as BC
import branch_spec as BS
import mode_seams as MS
import test_mode_seams_cpu as StandIns
from conftest import ROOT
from jaderaytracerendering_amd import _abi, backend as B

U32 = np.uint32


@pytest.fixture(scope="module")
def dbg():
    path = os.path.join(ROOT, "jaderaytracerendering_amd", "lib", "libjade_hip_debug.so")
    assert os.path.exists(path), "libjade_hip_debug.so missing: run `make hipvariants` (or __graft_entry__.build())"
    lib = C.CDLL(path)
    lib.jade_debug_branch_number_host.restype = C.c_int
    lib.jade_debug_branch_number_host.argtypes = [C.c_int32, C.c_void_p, C.c_void_p]
    lib.jade_debug_shade_mode_passes_host.restype = C.c_int
    lib.jade_debug_shade_mode_passes_host.argtypes = [C.c_int32] * 7 + [C.POINTER(C.c_uint32)]
    lib.jade_debug_shade_mode_branch_host.restype = C.c_int
    lib.jade_debug_shade_mode_branch_host.argtypes = [C.c_int32] * 8 + [C.POINTER(C.c_uint32)]
    lib.jade_last_error.restype = C.c_char_p
    return lib


# ------------------------------------------------------------------------------------------------------------------ the number --

def test_the_rows_are_the_ones_the_statement_is_held_on():
    r = BS.rows()
    s = set(r[:, 3].tolist())
    assert set(range(4096)) <= s and 2 ** 32 - 1 in s
    assert all(v in s for k in range(32) for v in (2 ** k, 2 ** k + 1, (2 ** k - 1) & 0xffffffff))
    assert {0, 1, 15, 16, 1919, 65535} <= set(r[:, 0].tolist()) and {0, 1, 15, 16, 1919, 65535} <= set(r[:, 1].tolist())
    assert len(set(r[:, 2].tolist())) >= 4 and set(r[:, 4].tolist()) == {0, 1}


def test_the_host_twin_is_the_statement_bit_for_bit(dbg):
    r = BS.rows()
    out = np.full(len(r), 0xdeadbeef, U32)
    assert dbg.jade_debug_branch_number_host(len(r), r.ctypes.data, out.ctypes.data) == _abi.JADE_OK
    want = BS.number_rows(r)
    bad = np.flatnonzero(out != want)
    assert len(bad) == 0, (len(bad), r[bad[:3]], out[bad[:3]], want[bad[:3]])
    # a depth the mode does not stratify is refused, not answered
    r2 = r[:2].copy()
    r2[1, 4] = 2
    assert dbg.jade_debug_branch_number_host(2, r2.ctypes.data, out.ctypes.data) == _abi.JADE_ERR_INVALID


def test_the_sequences_by_hand():
    assert BS.A([0, 1, 2, 3, 0x80000000, 0xffffffff]).tolist() == [0, 0x80000000, 0x40000000, 0xc0000000, 1, 0xffffffff]
    # Sobol's second dimension: direction numbers 0x80000000, 0xc0000000, 0xa0000000, 0xf0000000, ...
    assert BS.B([0, 1, 2, 3, 4, 8]).tolist() == [0, 0x80000000, 0xc0000000, 0x40000000, 0xa0000000, 0xf0000000]
    assert float(BS.su(U32(0))) == 0.0 and float(BS.su(U32(0xffffffff))) == 1.0 and float(BS.su(U32(0x80000000))) == 0.5
    assert BS.shl1(U32(0xc0000001)) == 0x80000002


def test_the_two_sequences_are_a_net_under_random_shifts():
    rng = np.random.default_rng(318)
    for k in range(0, 11):
        for _ in range(4):
            da, db = (int(v) for v in rng.integers(0, 2 ** 32, 2))
            blocks = [0] + [int(v) for v in rng.integers(0, 2 ** (32 - k), 3)]   # the first 2^k points, and aligned blocks of 2^k
            for blk in blocks:
                i = (np.arange(1 << k, dtype=np.uint64) + np.uint64(blk << k)) & np.uint64(0xffffffff)
                assert BS.is_net(BS.A(i) ^ U32(da), BS.B(i) ^ U32(db), k), (k, blk, da, db)
    # (the check can fail: the first dimension twice is no net)
    i = np.arange(16)
    assert not BS.is_net(BS.A(i), BS.A(i), 4)


def test_a_pixels_samples_share_out_the_arms():
    """Exactly N / 2 of a pixel's first N numbers fall below 0.5 (N = 2, 4, 8, 64), 2 or 3 of the first 5; of the 32 of 64 that do not, 28 or
    29 pass su(U << 1) < 0.9: the next five bits of U take every value once, 0.9 * 32 = 28.8."""
    rng = np.random.default_rng(17)
    px = np.concatenate([[(0, 0, 0), (1919, 1079, 7), (65535, 65535, 0xffffffff)], rng.integers(0, 2 ** 16, (200, 3))])
    seen = set()
    for x, y, frame in px:
        for d in (0, 1):
            for n in (2, 4, 8, 64):
                W = BS.U(x, y, frame, np.arange(n), d)
                assert int((BS.su(W) < np.float32(0.5)).sum()) == n // 2, (x, y, frame, d, n)
            arm, _, rr = BS.decisions(W, True)
            assert int((~arm).sum()) == 32 and int((~arm & rr).sum()) in (28, 29)
            seen.add(int((~arm & rr).sum()))
            low5 = int((BS.su(BS.U(x, y, frame, np.arange(5), d)) < np.float32(0.5)).sum())
            assert low5 in (2, 3)
            # the SSS select of the 32 that take the arm: sixteen each
            arm, sss, _ = BS.decisions(W, True)
            assert int((arm & sss).sum()) == 16
    assert seen == {28, 29}


def test_the_shift_is_uniform_over_pixels():
    y, x = np.mgrid[0:256, 0:256]
    for frame, sidx, d in ((0, 0, 0), (0, 0, 1), (1000, 3, 0), (7, 5, 1)):
        u = BS.su(BS.U(x.ravel(), y.ravel(), frame, sidx, d)).astype(np.float64)
        assert len(u) == 2 ** 16
        se = np.sqrt(1.0 / 12.0 / len(u))   # the standard error of the mean of 2^16 uniforms
        assert abs(u.mean() - 0.5) <= 4 * se, (frame, sidx, d, u.mean())


# ------------------------------------------------------------------------------------------------------------ shade_mode_for --
ENVIS, LENS, SHUTTER, LIGHTS, COSINE, MIS, ENVMIX, PASSES, BRANCH = (1 << i for i in range(9))
ENVS = (_abi.ENV_REFERENCE, _abi.ENV_IMPORTANCE, _abi.ENV_MIXTURE)
ALL = list(itertools.product(ENVS, (0, 1), (0, 1), (_abi.LIGHTS_ALL, _abi.LIGHTS_ONE), (_abi.BOUNCE_UNIFORM, _abi.BOUNCE_COSINE),
                             (_abi.DIRECT_RAYS, _abi.DIRECT_MIS), (0, 1)))


def _ask(dbg, combo, branch=None):
    mode = C.c_uint32(0xdeadbeef)
    rc = dbg.jade_debug_shade_mode_passes_host(*combo, C.byref(mode)) if branch is None else dbg.jade_debug_shade_mode_branch_host(*combo, branch, C.byref(mode))
    return rc, mode.value, (dbg.jade_last_error() or b"").decode()


def test_exactly_the_twelve_new_modes_are_accepted_beside_the_36_old_ones(dbg):
    assert len(ALL) == 192
    old, new = {}, {}
    for combo in ALL:
        before = _ask(dbg, combo)
        off = _ask(dbg, combo, _abi.BRANCH_RANDOM)
        assert off[:2] == before[:2] and (off[0] == _abi.JADE_OK or off[2] == before[2]), ("JADE_BRANCH_RANDOM answers as before", combo)
        if before[0] == _abi.JADE_OK:
            old[combo] = before[1]
        rc, mode, text = _ask(dbg, combo, _abi.BRANCH_STRATIFIED)
        env, lens, shutter, lights, bounce, direct, passes = combo
        if rc == _abi.JADE_OK:
            new[combo] = mode
            assert mode == old[combo] | BRANCH
            continue
        assert rc == _abi.JADE_ERR_UNSUPPORTED and mode == 0xdeadbeef, "refused, and the mode left alone"
        if before[0] != _abi.JADE_OK:
            assert text == before[2], "the other modes' refusals come first and keep their texts"
            continue
        assert text.startswith("branch sampling: JADE_BRANCH_STRATIFIED (jade_scene_set_branch_sampling)"), text
        word = "lens" if lens else "shutter" if shutter else "JADE_LIGHTS_ONE" if lights == _abi.LIGHTS_ONE else "passes"
        assert word in text, (combo, text)
        if word == "lens":
            assert "shutter" not in text, "a lens is named before a shutter, and only one of them"
    assert len(old) == 36 and len(new) == 12
    rows = ((_abi.BOUNCE_UNIFORM, _abi.DIRECT_RAYS, 0), (_abi.BOUNCE_COSINE, _abi.DIRECT_RAYS, 0), (_abi.BOUNCE_COSINE, _abi.DIRECT_MIS, 0),
            (_abi.BOUNCE_UNIFORM, _abi.DIRECT_RAYS, 1))
    assert set(new) == {(env, 0, 0, _abi.LIGHTS_ALL, b, d, p) for env in ENVS for b, d, p in rows}
    assert dbg.jade_debug_shade_mode_branch_host(0, 0, 0, 0, 0, 0, 0, 1, None) == _abi.JADE_ERR_INVALID
    for bad in (2, -1, 255):
        assert _ask(dbg, ALL[0], bad)[0] == _abi.JADE_ERR_INVALID


# ----------------------------------------------------------------------------------- what the device tests take from the statement --

def test_the_counting_scene_counts_what_the_shares_say():
    """At 2, 4, 8 and 64 spp exactly half the samples of every pixel take the sub-surface arm; at 5 spp two or three per pixel.  The frame
    the random render is held against misses 3072 by more than 20 at 2 spp (a binomial with standard deviation 39)."""
    for spp in (2, 4, 8, 64):
        sub, mir = BC.stratified_counts(BC.COUNT_FRAME, spp)
        assert sub == BC.COUNT_PIXELS * spp // 2
        assert abs(mir - 0.9 * (BC.COUNT_PIXELS * spp - sub)) <= 0.04 * BC.COUNT_PIXELS * spp
    sub5, _ = BC.stratified_counts(BC.COUNT_FRAME, 5)
    assert 2 * BC.COUNT_PIXELS <= sub5 <= 3 * BC.COUNT_PIXELS
    assert abs(BC.random_arm_count(BC.COUNT_FRAME, 2) - BC.COUNT_PIXELS) > 20


def test_every_ray_of_the_counting_scene_meets_the_triangle():
    """The statement's own camera rays, at the corners of the jitter: the triangle fills the frame."""
    import jade_spec
    S = jade_spec.Scene(BC.count_scene())
    eye, cam = BC.count_pose()
    for x, y in ((0, 0), (BC.COUNT_W - 1, 0), (0, BC.COUNT_H - 1), (BC.COUNT_W - 1, BC.COUNT_H - 1), (31, 20)):
        for s in range(4):
            tr = []
            jade_spec.sample(S, x, y, BC.COUNT_W, BC.COUNT_H, eye, cam, s, tr)
            assert tr and tr[0] != "sky" and len([t for t in tr if t in ("sss", "bssrdf", "mirror")]) == 1, (x, y, s, tr)


@pytest.mark.parametrize("name", list(BC.COMPARE))
def test_the_need_tables_are_half_of_what_the_statement_alone_counts(name):
    counts = BC.spec_counts(name)
    print(name, dict(sorted(counts.items())))
    assert BC.NEED[name] == {t: n // 2 for t, n in counts.items() if t in BC.NEED_TAGS}
    assert BC.NEED[name].get("branch-d0", 0) >= 30, "the camera vertex is met"
    for tag in BC.MUST_REACH[name]:
        assert BC.NEED[name].get(tag, 0) >= 5, (name, tag, counts)


def test_the_stratified_sample_is_the_random_one_with_three_draws_replaced():
    """stratified=False is jade_spec.sample on the same stream; and a vertex of depth >= 2 reads the stream in both."""
    import jade_spec
    hs, eye, cam, _ = BC.spec_samples("jade_cube")
    S = BS.scene("reference", hs)
    differ = 0
    for x, y in itertools.product(range(0, 12, 3), range(0, 12, 3)):
        a = BS.sample(S, x, y, 12, 12, eye, cam, 3, 2, [], stratified=False)
        b = jade_spec.sample(S, x, y, 12, 12, eye, cam, 5, [])
        assert np.array_equal(a, b)
        differ += not np.array_equal(a, BS.sample(S, x, y, 12, 12, eye, cam, 3, 2, []))
    assert differ > 0


# ------------------------------------------------------------------------------------------------------------------ the seams --

class Scene(StandIns.Scene):
    """test_mode_seams_cpu's stand-in with the branch setting: refused with a lens or a shutter by name, after the other modes' refusals;
    the list schedule - no inline rays."""

    def __init__(self, be, hs):
        super().__init__(be, hs)
        self.set["branch"] = 0

    branch_sampling = property(lambda self: self.set["branch"])
    set_branch_sampling = lambda self, v: self._mode("branch", v)  # noqa: E731

    def begin(self, p):
        super().begin(p)
        s = self.set
        camera = "a lens" if s["lens"][0] > 0 else "a shutter" if s["shutter"] is not None else None
        if camera and s["branch"]:
            del self.p
            StandIns._refuse(_abi.JADE_ERR_UNSUPPORTED, "branch sampling: JADE_BRANCH_STRATIFIED does not run together with " + camera)


class StandIn(StandIns.StandIn):
    def scene(self, hs):
        return Scene(self, hs)


def _render_multi(be, scenes, p):
    if any(s.set["branch"] != scenes[0].set["branch"] for s in scenes):
        StandIns._refuse(_abi.JADE_ERR_INVALID, "the scenes carry different branch sampling modes")
    return StandIns.render_multi(be, scenes, p)


CHECKS = dict(StandIns.CHECKS)
CHECKS["render_multi"] = lambda be, case, ref, mp: MS.check_render_multi(be, case, ref, render_multi=_render_multi)


def test_the_case_is_a_sampling_case_under_the_list_schedule():
    case = BC.CASE
    assert case.name == "branch" and case.knob == ("branch_sampling", "set_branch_sampling", _abi.BRANCH_STRATIFIED)
    assert case.name not in MS.BY_NAME and MS.schedules(case) == MS.COMMON_SCHEDULES
    n, spp = case.steps
    assert n * spp == case.params().spp and case.shares == 2 and case.invariants is MS.camera_invariants


def test_the_stand_in_passes_every_check(monkeypatch):
    case, be = BC.CASE, StandIn()
    ref = MS.reference(be, case)
    for name, check in CHECKS.items():
        check(be, case, ref, monkeypatch)
    MS.check_oracle_refuses(StandIns.Oracle(), case)
    with pytest.raises(AssertionError):
        MS.check_oracle_refuses(be, case)


@pytest.mark.parametrize("fault", StandIns.FAULTS)
def test_a_wrong_stand_in_is_caught_by_its_check(fault, monkeypatch):
    case, be = BC.CASE, StandIn(fault)
    ref = MS.reference(be, case)
    with pytest.raises(AssertionError):
        CHECKS[StandIns.CAUGHT_BY[fault]](be, case, ref, monkeypatch)


def test_the_python_names():
    assert (_abi.BRANCH_RANDOM, _abi.BRANCH_STRATIFIED) == (0, 1)
    assert callable(B.Scene.set_branch_sampling) and isinstance(B.Scene.branch_sampling, property)
    assert {"jade_scene_set_branch_sampling", "jade_scene_get_branch_sampling"} <= set(_abi.BVH_SYMBOLS)
