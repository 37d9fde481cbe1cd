"""JADE_BRANCH_STRATIFIED on the device (include/jade_bvh.h, "The branch draws, stated"; tests/branch_spec.py is that text in numpy).

1. The debug entry: branch_number on the device equals the statement on branch_spec.rows(), with no differing bit.
2. Off is today: JADE_BRANCH_RANDOM set explicitly is the untouched handle, frame bits and every integer of jade_stats, under the default
   schedule and under JADE_FUSED=0 JADE_TAIL=0, on tinyjade and on the two-lamps scene.
3. The arms are shared out, counted end to end on ONE sub-surface mirror triangle that fills a 64 x 48 frame: rays_env is the number of
   samples numpy says take the sub-surface arm - exactly half at 2, 4, 8 and 64 spp - and rays_mirror the number that take the mirror
   arm and pass su(U << 1) < 0.9.  The random render of the same frame does not meet the equality.
4. Against the float64 statement, sample for sample: sidx 0 .. 7 of every pixel one by one, with spec_scenes.compare_arm's bar.
5. Unbiased against the random mode: 64 frames of 64 spp from fixed seeds in both modes, the frame averages within 4 standard errors of
   the RANDOM mode's.
6. The seams: mode_seams' checks on the mode's case; passes, adaptive sampling, the denoiser, exposure and glare on top."""
import ctypes as C

import numpy as np
import pytest

import branch_cases as BC
import branch_spec as BS
import camera_cases
import mode_seams as MS
import spec_scenes as SP
from camera_cases import DEBUG_LIB, tinyjade
from jaderaytracerendering_amd import _abi, backend as B, host as H
from render_helpers import all_counters, same_bits, with_params

pytestmark = pytest.mark.gpu

STRAT, RANDOM = _abi.BRANCH_STRATIFIED, _abi.BRANCH_RANDOM
U24 = 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------ 1. the debug entry --

def test_the_device_forms_the_statements_number_bit_for_bit(hip):
    lib = C.CDLL(DEBUG_LIB)
    lib.jade_debug_branch_number.restype = C.c_int
    lib.jade_debug_branch_number.argtypes = [C.c_int, C.c_int32, C.c_void_p, C.c_void_p]
    r = BS.rows()
    out = np.full(len(r), 0xdeadbeef, np.uint32)
    assert lib.jade_debug_branch_number(0, len(r), r.ctypes.data, out.ctypes.data) == _abi.JADE_OK
    want = BS.number_rows(r)
    bad = np.flatnonzero(out != want)
    assert len(bad) == 0, (len(bad), r[bad[:3]], out[bad[:3]], want[bad[:3]])


# --------------------------------------------------------------------------------------------------------------- 2. off is today --

def _two_lamps():
    eye, cam = H.camera_orbit(2.8, 20.0, 10.0)
    return SP.build("two_lamps"), B.make_params(32, 24, 8, eye, cam, frame=3)


OFF_SCENES = {"tiny": lambda: tinyjade(8)[:2], "two_lamps": _two_lamps}


@pytest.mark.parametrize("schedule", [{}, {"JADE_FUSED": "0", "JADE_TAIL": "0"}], ids=["default", "FUSED=0,TAIL=0"])
@pytest.mark.parametrize("scene", list(OFF_SCENES))
def test_random_set_explicitly_is_the_untouched_handle(hip, monkeypatch, scene, schedule):
    for k, v in schedule.items():
        monkeypatch.setenv(k, v)
    hs, p = OFF_SCENES[scene]()
    with hip.scene(hs) as sc:
        assert sc.branch_sampling == RANDOM
        untouched = sc.render(p)
    with hip.scene(hs) as sc:
        sc.set_branch_sampling(STRAT)
        assert sc.branch_sampling == STRAT
        sc.set_branch_sampling(RANDOM)
        explicit = sc.render(p)
        sc.set_branch_sampling(STRAT)
        on = sc.render(p)
    assert same_bits(untouched[0], explicit[0]) and np.array_equal(untouched[1], explicit[1])
    assert all_counters(untouched[2]) == all_counters(explicit[2])
    if not schedule:
        assert untouched[2].rays_inline > 0, "the default schedule: the fused first pass ran"
    assert not same_bits(on[0], untouched[0]) and on[2].rays_inline == 0 and on[2].tail_launches == 0
    assert on[2].samples == untouched[2].samples == on[2].rays_primary


# ------------------------------------------------------------------------------------------ 3. the arms, counted end to end --

def _count(hip, mode, spp):
    eye, cam = BC.count_pose()
    p = B.make_params(BC.COUNT_W, BC.COUNT_H, spp, eye, cam, frame=BC.COUNT_FRAME)
    with hip.scene(BC.count_scene()) as sc:
        sc.set_branch_sampling(mode)
        _, _, st = sc.render(p, want_bgr8=False)
    assert st.samples == st.rays_primary == st.shaded_hits == BC.COUNT_PIXELS * spp, "every camera ray meets the triangle, and every path ends at it"
    return st


@pytest.mark.parametrize("spp", [2, 4, 5, 8, 64])
def test_the_arms_are_shared_out(hip, spp):
    sub, mir = BC.stratified_counts(BC.COUNT_FRAME, spp)
    if spp != 5:
        assert sub == BC.COUNT_PIXELS * spp // 2
    else:
        assert 2 * BC.COUNT_PIXELS <= sub <= 3 * BC.COUNT_PIXELS
    st = _count(hip, STRAT, spp)
    print(f"{spp} spp: rays_env {st.rays_env} (numpy {sub}), rays_mirror {st.rays_mirror} (numpy {mir})")
    assert st.rays_env == sub
    assert st.rays_mirror == mir
    assert st.rays_refract == 0 and st.rays_shadow == 0


def test_the_random_render_does_not_share_them_out(hip):
    st = _count(hip, RANDOM, 2)
    want = BC.random_arm_count(BC.COUNT_FRAME, 2)
    print(f"random, 2 spp: rays_env {st.rays_env} (the numpy stream {want}; the shared-out count {BC.COUNT_PIXELS})")
    assert abs(want - BC.COUNT_PIXELS) > 20
    assert st.rays_env == want and st.rays_env != BC.COUNT_PIXELS


# ------------------------------------------------------------------------------------- 4. the float64 statement, sample by sample --

def _device_samples(hip, name):
    """[sidx] -> float64 [SIZE, SIZE, 3]: sample sidx of every pixel, from the linear frame after every step of one sample:
    n mean_n - (n - 1) mean_(n-1).  Also the bound of that difference's error, per sample and pixel: below 1024 samples every partial-sum
    lane holds one sample and the resolve adds the lanes in ascending order, so S_n = fl(S_(n-1) + x_n) - one rounding, at most u S_n,
    u = 2^-24 - and mean_n = fl(S_n fl(1 / n)) - two more, so n mean_n is S_n within (2 u + u^2) S_n; the same for n - 1 with S_(n-1) <=
    S_n, no addend being negative in these scenes' samples.  Together at most (5 u + 2 u^2) S_n <= 6 u S_n; S_n itself is taken as
    n mean_n (1 + 3 u)."""
    c = BC.COMPARE[name]
    hs, eye, cam, _ = BC.spec_samples(name)
    frame, = c["frames"]
    out, bound = [], []
    with hip.scene(hs) as sc:
        for setter, value in c["modes"]:
            getattr(sc, setter)(value)
        sc.set_branch_sampling(STRAT)
        sc.begin(B.make_params(BC.SIZE, BC.SIZE, BC.SAMPLES, eye, cam, frame=frame, env_sampling=c["env"]))
        prev = np.zeros((BC.SIZE, BC.SIZE, 3))
        for n in range(1, BC.SAMPLES + 1):
            sc.step(1)
            s_n = n * sc.resolve(want_bgr8=False)[0].astype(np.float64)
            out.append(s_n - prev)
            bound.append(6 * U24 * np.abs(s_n) * (1 + 3 * U24))
            prev = s_n
    return out, bound


@pytest.mark.parametrize("name", list(BC.COMPARE))
def test_every_sample_is_the_statements(hip, name):
    """spec_scenes.compare_arm's bar - 1e-4 relative with a floor of 1e-3, at most 2 % of the samples disagreeing, coplanar BSSRDF exits
    left out, every tag of `need` reached by half of what the statement alone counts - on sidx 0 .. 7 one by one, the floor widened by
    the difference's own rounding bound (_device_samples)."""
    frame, = BC.COMPARE[name]["frames"]
    want_rows = BC.spec_samples(name)[3]
    got, bound = _device_samples(hip, name)
    seen, bad, n, skipped, worst = {}, [], 0, 0, 0.0
    for s in range(BC.SAMPLES):
        for x, y, tr, want in want_rows[frame, s]:
            if "bssrdf-coplanar" in tr:
                skipped += 1
                continue
            n += 1
            g = got[s][y, x]
            err = np.abs(g - want)
            if bool((err <= 1e-4 * np.maximum(np.abs(want), 1e-3) + bound[s][y, x]).all()):
                worst = max(worst, float((err / np.maximum(np.abs(want), 1e-3)).max()))
                for t in set(tr):
                    seen[t] = seen.get(t, 0) + 1
            else:
                bad.append((s, x, y, tr, g, want))
    print(f"compare {name}: {n} compared, {len(bad)} disagree, {skipped} left out, worst relative error {worst:.3g}, seen {dict(sorted(seen.items()))}")
    assert len(bad) <= 0.02 * n, f"{len(bad)} of {n} samples disagree with the statement, e.g. {bad[:3]}"
    for tag, count in BC.NEED[name].items():
        assert seen.get(tag, 0) >= count, f"only {seen.get(tag, 0)} agreeing samples went through '{tag}' ({seen})"


# --------------------------------------------------------------------------------------------- 5. unbiased against the random mode --

UNBIASED = {"tiny": lambda: tinyjade(64, 32, 24)[:2], "two_lamps": lambda: (_two_lamps()[0], with_params(_two_lamps()[1], spp=64))}
SEEDS = [1000 * k for k in range(64)]   # (a sample's stream is seeded frame + sidx: 64 samples apart is distinct)


@pytest.mark.parametrize("scene", list(UNBIASED))
def test_the_frame_average_is_the_random_modes(hip, scene):
    """Per channel, |mean over the 64 frames' averages, stratified - random| <= 4 sigma, sigma the standard error of the RANDOM mode's
    64 frame averages: the reference's scatter sets the bar."""
    hs, p = UNBIASED[scene]()
    avg = {}
    with hip.scene(hs) as sc:
        for mode in (RANDOM, STRAT):
            sc.set_branch_sampling(mode)
            avg[mode] = np.array([sc.render(with_params(p, frame=f), want_bgr8=False)[0].astype(np.float64).mean((0, 1)) for f in SEEDS])
    sigma = avg[RANDOM].std(0, ddof=1) / np.sqrt(len(SEEDS))
    diff = avg[STRAT].mean(0) - avg[RANDOM].mean(0)
    print(f"{scene}: random {avg[RANDOM].mean(0)}, stratified {avg[STRAT].mean(0)}, difference / sigma {diff / sigma}; "
          f"scatter of the frame averages, stratified / random {avg[STRAT].std(0, ddof=1) / avg[RANDOM].std(0, ddof=1)}")
    assert (sigma > 0).all() and (np.abs(diff) <= 4 * sigma).all(), (diff, sigma)


# ------------------------------------------------------------------------------------------------------------------ 6. the seams --
CASE = BC.CASE


@pytest.fixture
def ref(hip):
    return MS.reference(hip, CASE)


def test_the_same_bits_and_counters_twice(hip, ref):
    MS.check_twice(hip, CASE, ref)


def test_the_same_bits_under_the_three_walks(hip, ref):
    MS.check_walks(hip, CASE, ref)


def test_steps_and_a_flush_equal_one_call(hip, ref):
    MS.check_steps(hip, CASE, ref)


def test_tile_shares_assemble_to_the_frame(hip, ref):
    MS.check_shares(hip, CASE, ref)


@pytest.mark.parametrize("env", MS.schedules(CASE), ids=MS.schedule_id)
def test_schedules_are_one_result(hip, ref, monkeypatch, env):
    MS.check_schedule(hip, CASE, ref, env, monkeypatch.setenv)


def test_an_unknown_value_is_invalid_and_leaves_the_setting(hip):
    MS.check_unknown_value(hip, CASE)


def test_the_oracle_has_no_such_entry_point(oracle):
    MS.check_oracle_refuses(oracle, CASE)


def test_render_multi_takes_equal_settings_and_refuses_unequal_ones(hip, ref):
    MS.check_render_multi(hip, CASE, ref)


def test_a_refusal_leaves_the_handle_usable(hip, ref):
    MS.check_refusal_leaves_the_handle_usable(hip, CASE, ref)


def test_one_light_sampling_and_other_passes_are_refused_by_name(hip):
    with hip.scene(CASE.small_scene()) as sc:
        sc.set_branch_sampling(STRAT)
        sc.set_light_sampling(_abi.LIGHTS_ONE)
        MS.refused(lambda: sc.begin(CASE.params()), _abi.JADE_ERR_UNSUPPORTED, ("JADE_BRANCH_STRATIFIED", "JADE_LIGHTS_ONE"))
        sc.set_light_sampling(_abi.LIGHTS_ALL)
        sc.set_passes(True)
        sc.set_bounce_sampling(_abi.BOUNCE_COSINE)
        MS.refused(lambda: sc.begin(CASE.params()), _abi.JADE_ERR_UNSUPPORTED, ("JADE_BRANCH_STRATIFIED", "passes"))
        sc.set_passes(False)
        assert np.isfinite(sc.render(CASE.params())[0]).all(), "cosine bounces with the shared-out draws render"


def test_the_command_line(tmp_path):
    MS.check_command_line(CASE, tmp_path)


def test_the_passes_add_up_to_the_stratified_frame(hip, ref):
    """Passes on top: the frame is the stratified frame in every bit, and the 15 images add up to it within the passes' own bound: per
    pixel and channel 2 N 2^-24 |frame|, N = spp (2 x 128 + 3) the most addends a pixel can have (tests/test_gpu_passes.py, check 2)."""
    p = CASE.params()
    with hip.scene(CASE.scene()) as sc:
        CASE.apply(sc)
        sc.set_passes(True)
        rgb, bgr, st = sc.render(p)
        passes = sc.passes()
    assert same_bits(rgb, ref[0]) and all_counters(st) == all_counters(ref[2])
    assert list(passes) == list(_abi.PASS_NAMES)
    total = np.stack(list(passes.values())).astype(np.float64).sum(0)
    bound = 2 * p.spp * (2 * 128 + 3) * U24 * np.abs(rgb.astype(np.float64))
    err = np.abs(total - rgb.astype(np.float64))
    print(f"worst |sum of passes - frame| / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3g}")
    assert (err <= bound).all() and sum(bool(v.any()) for v in passes.values()) >= 8


def test_a_stopped_tile_is_the_uniform_stratified_render_at_its_count(hip):
    camera_cases.check_adaptive_tiles_equal_uniform_renders(hip, lambda sc: sc.set_branch_sampling(STRAT))


def test_the_denoiser_exposure_and_glare_run_on_top(hip):
    camera_cases.check_denoise_is_denoise_image_on_its_own_inputs(hip, lambda sc: sc.set_branch_sampling(STRAT))
    with hip.scene(CASE.scene()) as sc:
        CASE.apply(sc)
        rgb, _, _ = sc.render(CASE.params())
        assert np.isfinite(sc.denoise()[0]).all()
        exposed = sc.resolve(exposure="auto")
        assert np.isfinite(exposed[0]).all() and exposed[1].any()
        sc.meter()
        assert np.isfinite(sc.glare()[0]).all()
        assert same_bits(sc.resolve()[0], rgb), "none of them touches the render"
