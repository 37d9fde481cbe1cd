"""Multiple importance sampling of the emitters on the device (include/jade_bvh.h, "The direct light, stated";
jade_scene_set_direct_sampling): the weight function against tests/mis_spec.py within a derived bound, the anchors that are cosine's
render bit for bit, counters that are cosine's while the frames differ, the bound the mode exists for next to a lamp's contact edge, the
render against mis_spec's arm sample for sample (tests/mis_cases.py) and the integral it estimates (Welch's t against the cosine mode,
which is the parent's code).  The seams every mode is held to - twice, the walks, steps, tile shares, schedules, the refusals,
jade_render_multi, the command line - are in tests/test_gpu_mode_seams.py (case "MIS" of tests/mode_seams.py)."""
import ctypes as C
import math

import numpy as np
import pytest

import mis_cases as MC
import mis_spec as spec
import mode_seams as MS
import spec_scenes as SP
from conftest import B, counters
from jaderaytracerendering_amd import _abi
from lamp_scenes import lamp_scene, params
from render_helpers import all_counters, same_bits, welch_t

pytestmark = pytest.mark.gpu

F32 = np.float32
COS, UNI = _abi.BOUNCE_COSINE, _abi.BOUNCE_UNIFORM
MIS, RAYS = _abi.DIRECT_MIS, _abi.DIRECT_RAYS
ONE, ALL = _abi.LIGHTS_ONE, _abi.LIGHTS_ALL


# --------------------------------------------------------------------------------------- 1. the weight function against the statement --
# The bound, derived before any device run.  e = 2^-24, the relative error of one fp32 rounding.  A dot product of three fma steps
# carries an ABSOLUTE error of at most 3 e sum |a_i b_i|: relative to the dot itself that is d(a, b) = 3 e sum |a_i b_i| / |dot(a, b)|,
# unbounded as the vectors become perpendicular - so it is carried per row (dn for dot(n, l), dne for dot(ne, l)).  A sum of squares
# has no cancellation: 3 e.
#   rl = sqrt(ll): 1.5 e + e = 2.5 e.   sne = sqrt(nne), sqrt(nn): 2.5 e each.
#   pA = ((ll rl) sne) / (A |dot(ne, l)|):  3 + 2.5 + 1 + 2.5 + 1 (numerator) + 1 + dne (denominator) + 1 (quotient) = 12 e + dne;  PL = mu pA: 13 e + dne.
#   pB = |dot(n, l)| / ((rl sqrt(nn)) pi):  dn + 2.5 + 2.5 + 1 + 1 + 1 (quotient) = 8 e + dn.
#   r = pB / PL: 22 e + dn + dne =: rho_r (24 e taken).   w_L = 1 / (1 + r): with r' = r (1 + x), |x| <= rho_r:
#       |w' - w| = w w' r |x| <= w (1 - w) rho_r / (1 - rho_r);  the sum and the quotient round once each, on a number <= 1: + 2 e (4 e taken).
#   g_B = ((m (|dot(n, l)| / rl)) sne) / (PL + pB): numerator dn + 2.5 + 1 + 1 + 2.5 + 1 = 8 e + dn; the sum of two positive numbers carries at
#       most the larger relative error of the two plus its own rounding: 14 e + dne + dn; the quotient 1:  23 e + 2 dn + dne.
#   T_B = ((Le f) g_B) / fl(0.9): 3 more:  rho_T = 26 e + 2 dn + dne (28 e taken), relative, as rho_T / (1 - rho_T).
# Rows are built so that rho stays below 1 %: a grazing dot(ne, l) goes down to 2^-12 |ne| |l|, not to rounding noise.
E = 2.0 ** -24


def mis_terms_device(be, rows):
    fn = be.lib.jade_debug_mis_terms
    fn.restype, fn.argtypes = C.c_int, [C.c_int, C.c_int32, C.c_void_p, C.c_void_p]
    rows = np.ascontiguousarray(rows, F32)
    out = np.full((len(rows), 2), np.nan, F32)
    be.check(fn(0, len(rows), rows.ctypes.data, out.ctypes.data))
    return out[:, 0], out[:, 1]


def unit(v):
    return v / np.sqrt((v * v).sum(-1))[..., None]


def term_rows():
    """(rows [k, 14] fp32, exact [k] bool): random rows with |l| from 2^-20 to 2^20, non-unit normals, m 1..3, mu = m or down to 1e-6;
    grazing dot(ne, l) from 2^-1 to 2^-12; and rows whose result is exact - mu = m = 0, a normal without an axis, dot(ne, l) = 0 on the
    axes, PL overflowing fp32 - for which the device must give (1, 0) bit for bit."""
    rng = np.random.default_rng(1313)
    k = 6000
    n = unit(rng.normal(size=(k, 3))) * rng.choice([0.3, 1.0, 2.5], size=(k, 1))
    ne = unit(rng.normal(size=(k, 3))) * rng.choice([1.0, 1.7, 0.4], size=(k, 1))
    A = rng.uniform(0.01, 5, size=k)
    m = rng.integers(1, 4, size=k).astype(np.float64)
    mu = np.where(rng.random(k) < 0.5, m, 10.0 ** rng.uniform(-6, 0, size=k))
    mu[:8] = 1e-6
    l = unit(rng.normal(size=(k, 3))) * 2.0 ** rng.integers(-20, 21, size=(k, 1))
    l[:64] = unit(l[:64]) * 2.0 ** np.repeat([-20, 20], 32)[:, None]
    # grazing: l = t + c ne_hat with t perpendicular to ne, |t| = 1: dot(ne_hat, l_hat) ~ c
    g = np.arange(k) % 5 == 0
    t = unit(np.cross(ne[g], rng.normal(size=(g.sum(), 3))))
    c = 2.0 ** -rng.integers(1, 13, size=g.sum())
    l[g] = (t + c[:, None] * unit(ne[g])) * 2.0 ** rng.integers(-6, 7, size=(g.sum(), 1))
    Le, f = rng.uniform(0.1, 60, size=k), rng.uniform(0.05, 0.3, size=k)
    rows = np.concatenate([n, ne, A[:, None], m[:, None], mu[:, None], l, Le[:, None], f[:, None]], 1).astype(F32)
    r64 = rows.astype(np.float64)
    cos_n = np.abs((r64[:, 0:3] * r64[:, 9:12]).sum(-1)) / np.sqrt((r64[:, 0:3] ** 2).sum(-1) * (r64[:, 9:12] ** 2).sum(-1))
    cos_e = np.abs((r64[:, 3:6] * r64[:, 9:12]).sum(-1)) / np.sqrt((r64[:, 3:6] ** 2).sum(-1) * (r64[:, 9:12] ** 2).sum(-1))
    rows = rows[(cos_n > 2.0 ** -12) & (cos_e > 2.0 ** -13)]
    base = rows[:40].copy()
    ex = []
    z = base.copy(); z[:, 7:9] = 0; ex.append(z)                                      # m = mu = 0: not weighted
    for bad in ([0, 0, 0], [np.nan, 1, 0], [np.inf, 0, 0], [2.0 ** 70, 0, 0]):        # no axis: the cosine mode's fallback
        z = base[:8].copy(); z[:, 0:3] = F32(bad); ex.append(z)
    z = base[:12].copy(); z[:, 3:6] = F32([1.7, 0, 0]); z[:, 9:12] = F32([0, 1, 0]) * (2.0 ** np.arange(-6, 6))[:, None].astype(F32)
    z[:, 0:3] = F32([0.3, 0.8, 0.1]); ex.append(z)                                    # dot(ne, l) = 0 exactly: PL = inf
    z = base[:12].copy(); z[:, 6] = F32(1e-30); z[:, 9:12] = (unit(z[:, 9:12].astype(np.float64)) * 2.0 ** 20).astype(F32); ex.append(z)  # PL overflows
    exact = np.concatenate(ex)
    return np.concatenate([rows, exact]).astype(F32), np.concatenate([np.zeros(len(rows), bool), np.ones(len(exact), bool)])


def row_bounds(rows, w, T):
    r = rows.astype(np.float64)
    n, ne, l = r[:, 0:3], r[:, 3:6], r[:, 9:12]
    dn = 3 * E * np.abs(n * l).sum(-1) / np.abs((n * l).sum(-1))
    dne = 3 * E * np.abs(ne * l).sum(-1) / np.abs((ne * l).sum(-1))
    rho_r, rho_T = 24 * E + dn + dne, 28 * E + 2 * dn + dne
    return w * (1 - w) * rho_r / (1 - rho_r) + 4 * E, T * rho_T / (1 - rho_T) + 1e-37, np.maximum(rho_r, rho_T)


def test_device_terms_are_the_statement_within_the_derived_bound(hip_debug):
    rows, exact = term_rows()
    assert (~exact).sum() > 5000 and exact.sum() > 90
    w, T = mis_terms_device(hip_debug, rows)
    assert ((w >= 0) & (w <= 1)).all(), "w_L lies in [0, 1] on every row"
    assert (w[exact] == 1).all() and (T[exact] == 0).all(), "rows the statement makes exact: (1, 0) bit for bit"
    want_w, want_T = spec.terms_rows(rows[~exact])
    bw, bT, rho = row_bounds(rows[~exact], want_w, want_T)
    assert rho.max() < 0.01
    ew, eT = np.abs(w[~exact] - want_w), np.abs(T[~exact] - want_T)
    print(f"mis terms: {len(want_w)} rows; w_L worst error {ew.max():.3g} (its bound {bw[ew.argmax()]:.3g}), worst error / bound {np.max(ew / bw):.3f}; "
          f"T_B worst relative error {np.max(eT / np.maximum(want_T, 1e-37)):.3g}, worst error / bound {np.max(eT / bT):.3f}; "
          f"w_L spans {want_w.min():.3g} .. {want_w.max():.6g}")
    assert (ew <= bw).all(), rows[~exact][np.argmax(ew / bw)]
    assert (eT <= bT).all(), rows[~exact][np.argmax(eT / bT)]
    assert want_w.min() < 1e-3 and want_w.max() > 0.999, "both ends of the weight are reached"


# ---------------------------------------------------------------------------------------------------- 2. anchors, bit for bit --

def render(hip, p, direct=MIS, name="lamp", lights=ALL, hs=None):
    with hip.scene(hs if hs is not None else lamp_scene(name)) as sc:
        sc.set_bounce_sampling(COS)
        sc.set_direct_sampling(direct)
        sc.set_light_sampling(lights)
        return sc.render(p)


def _same(out, ref, what=""):
    assert same_bits(out[0], ref[0]) and np.array_equal(out[1], ref[1]), what
    assert all_counters(out[2]) == all_counters(ref[2]), what


def dark_list_scene():
    """The lamp scene with only triangles that do not emit listed (four of the slab's): entries, draws and shadow rays, nothing weighted."""
    base = lamp_scene("lamp")
    hs = type(base)({k: np.array(v, copy=True) for k, v in base.a.items()}, base.bvh_depth)
    dark = np.flatnonzero((base.tri_f32()[:, 13:16] == 0).all(1))[:4]
    hs.a["emit"] = np.int32(dark)
    return hs


@pytest.mark.parametrize("lights", [ALL, ONE])
def test_without_weighted_entries_the_mode_is_cosines_render_in_every_float_and_counter(hip, lights):
    for name, hs in (("none", lamp_scene("none")), ("non-emitters only", dark_list_scene())):
        if lights == ONE and len(hs.a["emit"]) == 0:
            continue
        _same(render(hip, params(), MIS, lights=lights, hs=hs), render(hip, params(), RAYS, lights=lights, hs=hs), name)


def test_the_default_mode_is_todays_render_after_a_round_trip(hip):
    with hip.scene(lamp_scene("lamp")) as sc:
        ref = sc.render(params())
        assert sc.direct_sampling == RAYS
        sc.set_bounce_sampling(COS)
        cos = sc.render(params())
        sc.set_direct_sampling(MIS)
        assert sc.direct_sampling == MIS
        sc.render(params(spp=1))
        sc.set_direct_sampling(RAYS)
        assert sc.direct_sampling == RAYS
        _same(sc.render(params()), cos, "cosine after the round trip")
        sc.set_bounce_sampling(UNI)
        back = sc.render(params())
    _same(back, ref, "the default after the round trip")
    assert ref[2].rays_inline > 0 and ref[2].tail_launches > 0, "the parent's schedule: fused first pass and tail kernel"


# ------------------------------------------------------------------------------------- 3. counters are cosine's --

@pytest.fixture(scope="module")
def mis_ref(hip):
    return render(hip, params())


@pytest.fixture(scope="module")
def cos_ref(hip):
    return render(hip, params(), RAYS)


def test_every_counter_is_cosines_while_the_frames_differ(mis_ref, cos_ref):
    assert counters(mis_ref[2]) == counters(cos_ref[2]), "rays, nodes, triangles, hits, samples: the rays are the same rays"
    assert all_counters(mis_ref[2]) == all_counters(cos_ref[2]), "every integer of jade_stats"
    assert np.isfinite(mis_ref[0]).all() and not same_bits(mis_ref[0], cos_ref[0])
    assert mis_ref[2].rays_inline > 0 and mis_ref[2].tail_launches == 0


@pytest.mark.parametrize("lights,envs", [(ONE, _abi.ENV_REFERENCE), (ALL, _abi.ENV_IMPORTANCE), (ONE, _abi.ENV_IMPORTANCE)])
def test_the_other_three_kernels_keep_cosines_counters_too(hip, lights, envs):
    p = params(env_sampling=envs)
    a, b = render(hip, p, MIS, lights=lights), render(hip, p, RAYS, lights=lights)
    assert counters(a[2]) == counters(b[2])
    assert np.isfinite(a[0]).all() and not same_bits(a[0], b[0])
    _same(render(hip, p, MIS, lights=lights), a, "twice")


@pytest.mark.parametrize("env", MS.COMMON_SCHEDULES[:2], ids=MS.schedule_id)
def test_records_per_pixel_and_the_unfused_first_pass_are_one_result(hip, mis_ref, monkeypatch, env):
    """Kept for its ids, which cannot all be retired in one change: tests/test_gpu_mode_seams.py runs this check for every case and environment."""
    MS.check_schedule(hip, MS.BY_NAME["MIS"], mis_ref, env, monkeypatch.setenv)


def test_adaptive_sampling_the_denoiser_and_environment_importance_run_on_top(hip):
    with hip.scene(lamp_scene("lamp")) as sc:
        sc.set_bounce_sampling(COS)
        sc.set_direct_sampling(MIS)
        rgb, bgr, tile_spp, st = sc.render_adaptive(params(spp=32), 8, 0.05)
        assert np.isfinite(rgb).all() and (tile_spp >= 8).all() and st.tail_launches == 0
        sc.render(params(spp=8, env_sampling=_abi.ENV_IMPORTANCE))
        dn, _ = sc.denoise()
        assert np.isfinite(dn).all() and dn.max() > 0


# ------------------------------------------------------------------------------------------------------------------ 4. the bound --
CONTACT_SEEDS = (0, 1, 2, 3, 4)   # chosen on the CPU with the two specs: cosine's largest floor sample is 4.4, 1.4, 11.2, 0.9, 2.0 x the bound


def contact_bound():
    """Per channel, from the statement alone.  A floor vertex (k = 1, unit normals, f = brdf fl(1 / pi)) gathers two emitter terms - the
    lamp's two triangles, each listed once: mu = 1 - of at most pi f Le |n| |ne| each, and a bounce term of at most pi f Le |n| |ne| m / RR:
    V = pi f Le (2 + 1 / 0.9).  A path's vertices add up with the indirect rate f (|n| / 2) / RR per vertex (the cosine mode's closed
    form), a geometric series: V / (1 - r).  1e-5 on top for fp32 rounding."""
    f = np.float64(SP.FLOOR["brdf"]) * float(F32(1.0 / spec.PI))
    V = math.pi * f * np.float64(MC.CONTACT_LE) * (2 + 1 / 0.9)
    r = f * 0.5 / 0.9
    return V / (1 - r) * (1 + 1e-5)


def test_next_to_the_contact_edge_every_floor_sample_is_bounded_where_cosines_is_not(hip):
    hs = MC.contact()
    eye, cam = MC.contact_camera()
    mask = MC.contact_floor_mask()
    assert 1000 < mask.sum() < 1300
    bound = contact_bound()
    worst_mis = worst_cos = 0.0
    with hip.scene(hs) as sc:
        sc.set_bounce_sampling(COS)
        for seed in CONTACT_SEEDS:
            p = B.make_params(MC.CONTACT_W, MC.CONTACT_H, 1, eye, cam, frame=seed)
            sc.set_direct_sampling(MIS)
            a, _, st_a = sc.render(p, want_bgr8=False)
            sc.set_direct_sampling(RAYS)
            b, _, st_b = sc.render(p, want_bgr8=False)
            assert counters(st_a) == counters(st_b)
            assert np.isfinite(a).all()
            worst_mis = max(worst_mis, float((a[mask].astype(np.float64) / bound).max()))
            worst_cos = max(worst_cos, float((b[mask].astype(np.float64) / bound).max()))
    print(f"contact edge: bound {bound}; largest floor sample / bound over {len(CONTACT_SEEDS)} seeds: mis {worst_mis:.3f}, cosine {worst_cos:.2f}")
    assert worst_mis <= 1.0
    assert worst_cos >= 10.0


# ------------------------------------------------------------------------------------------------------------------ 5. the cases --

@pytest.mark.parametrize("case", sorted(MC.CASES))
def test_the_render_is_the_statement_sample_for_sample(hip, case):
    MC.compare(hip, **MC.CASES[case])


# ------------------------------------------------------------------------------------------------------------ 6. the same integral --
WELCH_K = 8
WELCH_LIMIT = 4.5
WELCH_SPP = {"lamp": 8, "contact": 8}   # the smallest power of two at which both scaled groups are told apart (the test's docstring)


def welch_setup(scene):
    """(host scene, params(spp, frame), mask of the pixels that do not look into a lamp)."""
    if scene == "lamp":
        return lamp_scene("lamp"), (lambda spp, frame: params(spp=spp, frame=frame)), None
    eye, cam = MC.contact_camera()
    return MC.contact(), (lambda spp, frame: B.make_params(MC.CONTACT_W, MC.CONTACT_H, spp, eye, cam, frame=frame)), MC.contact_floor_mask()


def welch_totals(hip, scene, spp):
    """Per mode, WELCH_K totals of radiance over the pixels that do not look into a lamp (the lamp scene: test_gpu_lights' mask, every
    channel below 4 in a frame of other samples; the contact scene: its floor mask), frames of independent samples, both modes from the
    same seeds."""
    hs, make, mask = welch_setup(scene)
    with hip.scene(hs) as sc:
        sc.set_bounce_sampling(COS)
        if mask is None:
            mask = (sc.render(make(64, 500000))[0] < 4).all(-1)
            assert 0.5 < mask.mean() < 1
        totals = {}
        for mode in (RAYS, MIS):
            sc.set_direct_sampling(mode)
            totals[mode] = [float(sc.render(make(spp, 1000 * k))[0].astype(np.float64)[mask].sum()) for k in range(WELCH_K)]
    return totals[RAYS], totals[MIS]


def welch_line(hip, scene, spp):
    c, m = welch_totals(hip, scene, spp)
    t, t_up, t_down = welch_t(c, m), welch_t(c, np.array(m) * 1.03), welch_t(np.array(c) * 1.03, m)
    print(f"welch {scene}: spp {spp}  cosine {np.mean(c):.6g} +- {np.std(c, ddof=1):.3g}  mis {np.mean(m):.6g} +- {np.std(m, ddof=1):.3g}  "
          f"t {t:+.3f}  mis x 1.03: {t_up:+.3f}  cosine x 1.03: {t_down:+.3f}")
    return t, t_up, t_down


@pytest.mark.parametrize("scene", ["lamp", "contact"])
def test_both_modes_estimate_the_same_integral(hip, scene):
    """Welch's t of eight totals per mode, |t| < 4.5; with either group scaled by 1.03 the same statistic must exceed 4.5, or the test
    could not fail.  The seeds are fixed: every run gives the same numbers.  WELCH_SPP is the smallest power of two at which both scaled
    groups lie beyond 4.5, measured once on an MI355X across 1 .. 64 spp (DESIGN.md 3.13 has the table): (t, t with mis x 1.03, t with
    cosine x 1.03) at 1 / 2 / 4 / 8 / 16 / 32 / 64 spp -
    lamp: (+0.00, -2.71, +2.72) (-0.00, -3.13, +3.13) (-0.00, -4.17, +4.17) (+0.00, -8.25, +8.26) (-0.01, -12.73, +12.71) (-0.02, -16.32, +16.29)
    (-0.02, -18.92, +18.89); totals at 8 spp: cosine 2882.72 +- 20.7, mis 2882.68 +- 20.7 - the lamps are small and far, the weights near 1;
    contact: (-0.23, -2.04, +1.56) (+0.23, -1.79, +2.23) (-0.41, -2.92, +2.04) (+0.09, -5.37, +5.45) (+0.24, -5.15, +5.49) (-0.39, -6.97, +6.04)
    (-0.48, -10.78, +9.56); totals at 8 spp: cosine 3209.19 +- 44.1, mis 3207.68 +- 22.6."""
    t, t_up, t_down = welch_line(hip, scene, WELCH_SPP[scene])
    assert abs(t) < WELCH_LIMIT
    assert abs(t_up) > WELCH_LIMIT and abs(t_down) > WELCH_LIMIT
