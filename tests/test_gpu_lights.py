"""One-light sampling on the device (include/jade_bvh.h, "The lights, stated"; jade_scene_set_light_sampling): the draw against
tests/lights_spec.py bit for bit, the two anchors (no emitter entry: JADE_LIGHTS_ALL's render; the default mode: today's), what the frame
and its counters are next to all lights', the work and the memory the mode is for, the integral it estimates, and (section 7) the render
against tests/jade_spec.py's one-light arm, sample for sample: how the shading kernels USE a draw.  The seams every mode is held to -
twice, the walks, steps, tile shares, schedules, the refusals, jade_render_multi, the command line - are in
tests/test_gpu_mode_seams.py (case "one-light" of tests/mode_seams.py)."""
import numpy as np
import pytest

import lights_spec as spec
import mode_seams as MS
import spec_scenes as SP
from conftest import B, counters
from jaderaytracerendering_amd import _abi, host as H
from lamp_scenes import HH, SPP, W, lamp_scene, params
from render_helpers import all_counters, same_bits, welch_t

pytestmark = pytest.mark.gpu


def render(hip, name, p, mode):
    with hip.scene(lamp_scene(name)) as sc:
        sc.set_light_sampling(mode)
        return sc.render(p)


@pytest.fixture(scope="module")
def one_ref(hip):
    """The lamp scene, one light per vertex, 6 spp: what the invariants below compare with."""
    return render(hip, "lamp", params(), _abi.LIGHTS_ONE)


@pytest.fixture(scope="module")
def all_ref(hip):
    return render(hip, "lamp", params(), _abi.LIGHTS_ALL)


# ------------------------------------------------------------------------------------------------------ 1. the draw, bit for bit --

def _rows(table, n_random=4096):
    """Uniforms [n, 4]: random rows, every slot with u2 exactly at, just below and just above its accept, u1 in {0, 1.0f} and at every slot
    boundary, (u3, u4) on both sides of the fold and on it."""
    n = len(table)
    rng = np.random.default_rng(5 + n)
    u = rng.random((n_random, 4)).astype(np.float32)
    one = np.float32(1)
    edge = []
    for s in range(n):
        u1 = np.float32((s + 0.5) / n)
        acc = table["accept"][s]
        for u2 in (acc, np.nextafter(acc, np.float32(-1)), np.nextafter(acc, np.float32(2)), np.float32(0), one):
            edge.append((u1, min(max(u2, np.float32(0)), one), rng.random(dtype=np.float32), rng.random(dtype=np.float32)))
        b = np.float32(s / n)
        for u1b in (b, np.nextafter(b, np.float32(-1)), np.nextafter(b, np.float32(2))):
            edge.append((min(max(u1b, np.float32(0)), one), rng.random(dtype=np.float32), rng.random(dtype=np.float32), rng.random(dtype=np.float32)))
    for u1 in (np.float32(0), one):
        for u3, u4 in ((0.5, 0.5), (0.25, 0.75), (1, 1), (0, 0), (1, 0), (0.75, 0.2500001), (0.6, 0.7), (1, 1e-30)):
            edge.append((u1, rng.random(dtype=np.float32), np.float32(u3), np.float32(u4)))
    return np.concatenate([u, np.array(edge, np.float32)])


@pytest.mark.parametrize("name", ["lamp1", "lamp3", "lamp82"])
def test_device_draw_equals_the_statement_bit_for_bit(hip_debug, name):
    hs = lamp_scene(name)
    n = len(hs.a["emit"])
    assert n == {"lamp1": 1, "lamp3": 3, "lamp82": 82}[name]
    table = spec.table_of(hip_debug.lib, hs.tri_f32(), hs.a["emit"])
    p = spec.weights(hs.tri_f32(), hs.a["emit"])
    assert np.abs(spec.implied(table) - p).max() < 1e-6
    u = _rows(table)
    assert len(u) >= 4096 and (u[:, 0] == 0).any() and (u[:, 0] == 1).any()
    assert n == 1 or (u[:, 1] == table["accept"][spec.slot_of(u[:, 0], n)]).sum() >= n
    with hip_debug.scene(hs) as sc:
        entry, rx, ry, w_draw, w_entry = spec.sample_device(sc, u)
    want_entry, own, want_rx, want_ry, want_w = spec.draw_f32(table, *u.T)
    bad = np.flatnonzero(entry != want_entry)
    assert len(bad) == 0, (len(bad), u[bad[0]], entry[bad[0]], want_entry[bad[0]])
    assert same_bits(rx, want_rx) and same_bits(ry, want_ry)
    assert same_bits(w_draw, want_w), np.flatnonzero(w_draw != want_w)[:5]
    assert same_bits(w_entry, want_w), "consume forms the weight again from the entry alone: the same float"
    assert (rx + ry <= 1).all() and (rx >= 0).all() and (ry >= 0).all()
    if n > 1:
        assert own.any() and (~own).any()


def test_device_draw_refuses_a_scene_without_entries(hip_debug):
    with hip_debug.scene(lamp_scene("none")) as sc:
        with pytest.raises(B.JadeError) as ei:
            spec.sample_device(sc, np.zeros((4, 4), np.float32))
    assert ei.value.code == _abi.JADE_ERR_UNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------- 2. the anchors --

def test_without_emitter_entries_one_light_is_all_lights_in_every_float_and_counter(hip):
    p = params()
    a = render(hip, "none", p, _abi.LIGHTS_ALL)
    o = render(hip, "none", p, _abi.LIGHTS_ONE)
    assert same_bits(a[0], o[0]) and np.array_equal(a[1], o[1])
    assert counters(a[2]) == counters(o[2]) and a[2].rays_shadow == 0


def test_the_default_mode_is_todays_render_after_a_round_trip(hip, all_ref):
    hs = lamp_scene("lamp")
    with hip.scene(hs) as sc:
        assert sc.light_sampling == _abi.LIGHTS_ALL
        fresh = sc.render(params())
    with hip.scene(hs) as sc:
        sc.set_light_sampling(_abi.LIGHTS_ONE)
        assert sc.light_sampling == _abi.LIGHTS_ONE
        sc.set_light_sampling(_abi.LIGHTS_ALL)
        assert sc.light_sampling == _abi.LIGHTS_ALL
        back = sc.render(params())
    for got in (fresh, back):
        assert same_bits(got[0], all_ref[0]) and np.array_equal(got[1], all_ref[1])
        assert all_counters(got[2]) == all_counters(all_ref[2])
    assert fresh[2].rays_inline > 0, "the fused first pass runs"


# ------------------------------------------------------------------------------------------------------------- 3. the frame --

def test_the_frame_is_finite_lit_and_not_all_lights(one_ref, all_ref):
    rgb, bgr, st = one_ref
    assert np.isfinite(rgb).all() and rgb.max() > 0 and st.samples == W * HH * SPP
    assert not same_bits(rgb, all_ref[0])
    assert st.rays_inline > 0 and st.tail_launches == 0, "the fused first pass stays, the tail kernel does not run"
    # the camera rays and what they meet are the same in both modes
    assert st.rays_primary == all_ref[2].rays_primary


@pytest.mark.parametrize("env", MS.COMMON_SCHEDULES, ids=MS.schedule_id)
def test_records_per_pixel_and_schedules_are_one_result(hip, one_ref, monkeypatch, env):
    """Kept for its ids, which cannot all be retired in one change: tests/test_gpu_mode_seams.py runs this check for every case and environment."""
    MS.check_schedule(hip, MS.BY_NAME["one-light"], one_ref, env, monkeypatch.setenv)


def test_secondary_rays_are_the_sum_of_their_five_parts(one_ref):
    st = one_ref[2]
    assert st.rays_secondary == st.rays_shadow + st.rays_env + st.rays_indirect + st.rays_mirror + st.rays_refract
    assert min(st.rays_shadow, st.rays_env, st.rays_indirect, st.rays_mirror) > 0


def test_with_environment_importance_on_top(hip, one_ref):
    p = params(env_sampling=_abi.ENV_IMPORTANCE)
    a = render(hip, "lamp", p, _abi.LIGHTS_ONE)
    b = render(hip, "lamp", p, _abi.LIGHTS_ONE)
    assert same_bits(a[0], b[0]) and counters(a[2]) == counters(b[2])
    assert np.isfinite(a[0]).all() and not same_bits(a[0], one_ref[0])
    st = a[2]
    assert st.rays_secondary == st.rays_shadow + st.rays_env + st.rays_indirect + st.rays_mirror + st.rays_refract
    # at most one shadow ray per sampling vertex; a vertex whose sky direction lay on the wrong side has no environment ray, so the
    # vertices are counted by the all-lights render of the same mode: 84 slots each, of which the side test drops some
    assert 0 < st.rays_shadow and st.tail_launches == 0


def test_adaptive_sampling_and_the_denoiser_run_on_top(hip):
    with hip.scene(lamp_scene("lamp")) as sc:
        sc.set_light_sampling(_abi.LIGHTS_ONE)
        rgb, bgr, tile_spp, st = sc.render_adaptive(params(spp=32), 8, 0.05)
        assert np.isfinite(rgb).all() and (tile_spp >= 8).all() and st.tail_launches == 0
        sc.render(params(spp=8))
        dn, _ = sc.denoise()
        assert np.isfinite(dn).all() and dn.max() > 0


# ------------------------------------------------------------------------------------------------------------------- 4. the work --

def test_at_most_one_shadow_ray_per_sampling_vertex(one_ref, all_ref):
    """JADE_ENV_REFERENCE sends one environment ray per sampling vertex, so rays_env counts the vertices."""
    one, al = one_ref[2], all_ref[2]
    assert 0 < one.rays_shadow <= one.rays_env
    assert al.rays_shadow > al.rays_env
    assert al.rays_shadow <= 84 * al.rays_env


# ----------------------------------------------------------------------------------------------------------------- 5. the memory --

def _bytes_per_record(n_shadow_slots):
    """jade_render_begin: bytes_per_record = 4 (34 + 5 nslots) + 6 nslots with nslots = shadow slots + 2 (ray records on, the default)."""
    nslots = n_shadow_slots + 2
    return 4 * (34 + 5 * nslots) + 6 * nslots


def test_records_per_pixel_do_not_fall_with_the_emitter_count(hip):
    """Under one fixed max_state_bytes the 81 924-entry scene gets at least the records per pixel in this mode that the 82-entry
    scene gets with all lights.  The bound is chosen so that the 82-entry scene's all-lights records (84 slots) fit 16 times per
    pixel and not 32 times: partial sums 12 x 64 lanes x npx, records npx x rpp x bytes_per_record."""
    spp = 64
    npx = ((W + 15) // 16) * ((HH + 15) // 16) * 256
    budget = 12 * 64 * npx + npx * 16 * _bytes_per_record(82) + 4096
    assert budget < 12 * 64 * npx + npx * 32 * _bytes_per_record(82)
    p = params(spp=spp)
    p.max_state_bytes = budget
    with hip.scene(lamp_scene("lamp82")) as sc:
        sc.begin(p)
        rpp_all_82 = sc.query(_abi.Q_RECORDS_PER_PIXEL)
    with hip.scene(lamp_scene("big")) as sc:
        sc.set_light_sampling(_abi.LIGHTS_ONE)
        sc.begin(p)
        rpp_one_big = sc.query(_abi.Q_RECORDS_PER_PIXEL)
    assert rpp_all_82 == 16
    assert rpp_one_big >= rpp_all_82 and rpp_one_big == 64


def test_a_frame_all_lights_has_no_memory_for_renders_with_one_light(hip):
    """max_state_bytes = twice what this mode needs for 256 x 256 at one record per pixel: partial sums 12 x 1 lane x npx + npx x
    bytes_per_record(1 shadow slot) = 4 (34 + 5 x 3) + 6 x 3 = 214 bytes.  With all lights one record has 81 926 slots, 2.13 MB: a 64 x 64
    frame's 4 096 records are 8.7 GB and JADE_ERR_NOMEM under that bound, and 256 x 256 is refused outright (the 32-bit slot index)."""
    npx = 256 * 256
    budget = 2 * (12 * npx + npx * _bytes_per_record(1))
    assert _bytes_per_record(1) == 214
    assert 64 * 64 * _bytes_per_record(81924) > budget and 64 * 64 * (81924 + 2) < 2 ** 32 <= npx * (81924 + 2)
    with hip.scene(lamp_scene("big")) as sc:
        small = params(spp=1, w=64, h=64)
        small.max_state_bytes = budget
        with pytest.raises(B.JadeError) as ei:
            sc.begin(small)
        assert ei.value.code == _abi.JADE_ERR_NOMEM
        large = params(spp=1, w=256, h=256)
        large.max_state_bytes = budget
        with pytest.raises(B.JadeError) as ei:
            sc.begin(large)
        assert ei.value.code == _abi.JADE_ERR_UNSUPPORTED
        sc.set_light_sampling(_abi.LIGHTS_ONE)
        rgb, bgr, st = sc.render(large)
        assert sc.query(_abi.Q_RECORDS_PER_PIXEL) == 1
    assert st.samples == 256 * 256 and np.isfinite(rgb).all() and rgb.max() > 0
    assert 0 < st.rays_shadow <= st.rays_env


# ----------------------------------------------------------------------------------------------------------- 6. the same integral --

WELCH_K = 8
WELCH_SPP = 8      # the smallest power of two at which the scaled group is told apart (measured: see the test's docstring)
WELCH_LIMIT = 4.5


def welch_totals(hip, spp):
    """Per mode, the WELCH_K totals of radiance over the lit pixels: frames of independent samples (frame = 1000 k), both modes from the
    same seeds.  Lit pixels: those that do not look straight into a lamp - every channel below 4, the weakest lamp channel - in an
    all-lights frame of other samples (frame = 500 000); the same pixels for every frame of both groups."""
    hs = lamp_scene("lamp")
    with hip.scene(hs) as sc:
        mask = (sc.render(params(spp=64, frame=500000))[0] < 4).all(-1)
        assert 0.5 < mask.mean() < 1
        totals = {}
        for mode in (_abi.LIGHTS_ALL, _abi.LIGHTS_ONE):
            sc.set_light_sampling(mode)
            totals[mode] = [float(sc.render(params(spp=spp, frame=1000 * k))[0].astype(np.float64)[mask].sum()) for k in range(WELCH_K)]
    return totals[_abi.LIGHTS_ALL], totals[_abi.LIGHTS_ONE]


def test_both_modes_estimate_the_same_integral(hip):
    """Welch's t of eight totals per mode, |t| < 4.5 (two-sided p about 5e-4 at these degrees of freedom); with one group scaled by
    1.03 the same statistic must exceed 4.5, or the test could not fail.  The seeds are fixed: every run gives the same numbers.
    Measured on an MI355X, (t, t with one light x 1.03, t with all lights x 1.03) at 1 / 2 / 4 / 8 / 16 / 32 / 64 spp:
    (-0.59, -3.10, +1.93) (-0.18, -3.56, +3.23) (+0.40, -4.23, +5.08) (+0.64, -8.82, +10.22) (+0.75, -11.16, +12.68) (-0.03, -15.96, +15.74)
    (-0.41, -24.21, +23.18): 8 spp is the smallest power of two at which both scaled groups are told apart.  Totals at 8 spp: all
    lights 2880.9 +- 12.8, one light 2875.2 +- 21.8."""
    a, o = welch_totals(hip, WELCH_SPP)
    t = welch_t(a, o)
    t_up = welch_t(a, np.array(o) * 1.03)
    t_down = welch_t(np.array(a) * 1.03, o)
    print(f"welch: spp {WELCH_SPP}  all {np.mean(a):.6g} +- {np.std(a, ddof=1):.3g}  one {np.mean(o):.6g} +- {np.std(o, ddof=1):.3g}  "
          f"t {t:+.3f}  one x 1.03: {t_up:+.3f}  all x 1.03: {t_down:+.3f}")
    assert abs(t) < WELCH_LIMIT
    assert abs(t_up) > WELCH_LIMIT and abs(t_down) > WELCH_LIMIT


# ------------------------------------------------------------------------ 7. the render against the float64 statement, sample for sample --
# How bounce_branch and consume USE a draw under SM_LIGHTS: jade_spec's one-light arm (include/jade_bvh.h's text in float64; checked
# without a GPU in tests/test_lights_spec_cpu.py) against 12 x 12 frames at 1 spp, by spec_scenes.compare and its bar, unchanged: a
# sample agrees when every channel is within 1e-4 relative (floor 1e-3), at most 2 % may disagree, bssrdf-coplanar samples are left out
# (here: at most 5 % of a case).

_checked = {}


def checked(hip, case):
    """compare() of one case of SP.LIGHT_CASES, once per session: (seen, bad, n, skipped, {"frames", "worst"})."""
    if case not in _checked:
        c = SP.LIGHT_CASES[case]
        out = {}
        r = SP.compare(hip, c["kind"], c["size"], c["frames"], c["need"], sky=c.get("sky", False), env_sampling=c.get("env_sampling", _abi.ENV_REFERENCE),
                       light_sampling=_abi.LIGHTS_ONE, max_left_out=0.05, out=out)
        _checked[case] = r + (out,)
    return _checked[case]


def one_light_frames(hip, case, kind=None):
    """The frames of a case as compare renders them, from a scene handle of its own (kind: another emitter list of the same geometry)."""
    c = SP.LIGHT_CASES[case]
    eye, cam = H.camera_orbit(2.8, 20.0, 10.0)
    with hip.scene(SP.build(kind or c["kind"], c.get("sky", False))) as sc:
        sc.set_light_sampling(_abi.LIGHTS_ONE)
        return {f: sc.render(B.make_params(c["size"], c["size"], 1, eye, cam, frame=f, threads=2, env_sampling=c.get("env_sampling", _abi.ENV_REFERENCE)),
                             want_bgr8=False)[0] for f in c["frames"]}


@pytest.mark.parametrize("case", sorted(SP.LIGHT_CASES))
def test_the_render_is_the_float64_statement_sample_for_sample(hip, case):
    """two_lamps: two lamps of unequal power, a duplicate entry and a listed non-emitter (own and alias, the side test's `continue`, lit
    and shadowed, in the diffuse, SSS-diffuse and BSSRDF branch); ..._sky and ..._sky_importance: under the textured sky in both
    env_sampling modes - k_shade_mode<ENVIS|LIGHTS>, four light draws before four environment draws; one_entry: nE = 1, weight exactly 1, only the
    four-for-two draw count differs from all lights; fan: 24 entries over 3.4 orders of magnitude, weights above 100, aliases
    frequent, a lit sample with a weight above 50 must agree; dark_list: only non-emitters listed - every term is zero and the draws
    still move everything behind them.

    Measured on the MI355X, samples compared / disagreeing / left out, and the worst relative error of an agreeing sample:
    two_lamps 560 / 0 / 16, 3.1e-6; two_lamps_sky 422 / 0 / 10, 4.6e-6; two_lamps_sky_importance 421 / 0 / 11, 7.7e-6; one_entry 422 / 0 / 10,
    3.1e-6; fan 560 / 0 / 16, 1.7e-5; dark_list 422 / 0 / 10, 1.7e-5 (the bar is 1e-4; the all-lights cases' worst is 5e-6)."""
    seen, bad, n, skipped, out = checked(hip, case)
    assert n + skipped == len(SP.LIGHT_CASES[case]["frames"]) * 144
    assert out["worst"] <= 1e-4


def test_a_dark_list_still_moves_the_draws(hip):
    """Every term of the dark list is zero, so its frames and the frames of the same triangles with NO list gather the same light - from
    other draws: four uniforms per sampling vertex against none."""
    _, _, _, _, out = checked(hip, "dark_list")
    bare = one_light_frames(hip, "dark_list", kind="no_list")
    for f, rgb in out["frames"].items():
        assert not same_bits(rgb, bare[f])


@pytest.mark.parametrize("env", [dict(JADE_FUSED="0"), dict(JADE_SORT="1", JADE_SORT_MIN="64"), dict(JADE_RECORDS_PER_PIXEL="1")], ids=lambda e: ",".join(f"{k[5:]}={v}" for k, v in e.items()))
def test_the_checked_frames_are_the_same_bits_under_other_schedules(hip, monkeypatch, env):
    """The unfused first pass, ordered queues and one record per pixel give the very arrays that were compared with the statement: the
    schedule matrix of tests/test_gpu_mode_seams.py hangs on a frame that has been checked."""
    _, _, _, _, out = checked(hip, "two_lamps")
    for k, v in env.items():
        monkeypatch.setenv(k, v)  # (read once, at jade_scene_create)
    again = one_light_frames(hip, "two_lamps")
    for f, rgb in out["frames"].items():
        assert same_bits(again[f], rgb), (env, f)
