"""The light passes on the device (include/jade_bvh.h, "The passes, stated"): jade_scene_set_passes, jade_render_passes.

1. Anchor: with passes on, the frame and every integer of jade_stats are those of the same render with passes off under the list schedule a
   passes render runs (JADE_FUSED=0 JADE_TAIL=0), bit for bit; set and unset, the default render is what it was.
2. Sum: per pixel and channel |sum of the passes - frame| <= 2 N 2^-24 |frame|, N = spp (2 x 128 + 3) the most addends a pixel can have
   (per sample: le, at most 128 pushed vertices of two parts each, the last l_dir's two parts).  Both sides are float32 sums of the same
   addends in another order, each within (N - 1) 2^-24 of the exact sum relative to the sum of |addend|, which is the frame where no
   addend is negative.  Negative addends come from schlick_out alone - the BSSRDF branch and the refraction loop; tests/test_passes_cpu.py - where the sum of
   |addend| is larger than the frame: there |frame| makes the bound asserted tighter than the one derived, never wider; the spec cases
   (check 3's scenes) are held to the derived bound with the statement's own sum of |addend|.
3. The float64 statement: tests/passes_spec.py's cases - the reference estimator, cosine bounces and MIS - pass by pass, with
   spec_scenes.compare's bar.
4. Seams: a mode_seams.Case for passes handed to mode_seams' checks through a backend whose frames carry the 15 pass images under the
   frame, so every assertion on a frame is an assertion on the passes too.
5. On top: adaptive sampling, jade_render_passes between steps, the denoiser, exposure and glare."""
import subprocess

import numpy as np
import pytest

import lamp_scenes
import mode_seams as MS
import passes_spec as PS
import scene_shapes
from jaderaytracerendering_amd import _abi, backend as B
from render_helpers import CLI, all_counters, read_pfm, same_bits, with_params

pytestmark = pytest.mark.gpu

NAMES = _abi.PASS_NAMES
U = 2.0 ** -24
W, H, SPP = 40, 36, 6   # edge tiles in both directions

COS, UNI, MIS, RAYS = _abi.BOUNCE_COSINE, _abi.BOUNCE_UNIFORM, _abi.DIRECT_MIS, _abi.DIRECT_RAYS
ESTIMATORS = {"reference": (UNI, RAYS), "cosine": (COS, RAYS), "MIS": (COS, MIS)}
SCENES = {"lamp": (lambda: lamp_scenes.lamp_scene("lamp"), lambda **kw: lamp_scenes.params(spp=SPP, w=W, h=H, **kw)),
          "base": (scene_shapes.base, lambda **kw: with_params(scene_shapes.params(), width=W, height=H, spp=SPP, **kw))}


def addends(spp):
    return spp * (2 * 128 + 3)


def set_estimator(sc, name):
    bounce, direct = ESTIMATORS[name]
    sc.set_bounce_sampling(bounce)
    sc.set_direct_sampling(direct)


def render_with_passes(hip, hs, p, estimator="reference"):
    with hip.scene(hs) as sc:
        set_estimator(sc, estimator)
        sc.set_passes(True)
        assert sc.passes_enabled
        rgb, bgr, st = sc.render(p)
        return rgb, bgr, st, sc.passes()


def stacked(passes):
    return np.stack([passes[n] for n in NAMES])


def check_sum(rgb, passes, spp, scale=None, what=""):
    """Check 2.  scale: the per-pixel sum of |addend| (default: |frame|)."""
    assert list(passes) == list(NAMES)
    total = stacked(passes).astype(np.float64).sum(0)
    assert np.isfinite(rgb).all() and np.isfinite(total).all(), what
    bound = 2 * addends(spp) * U * (np.abs(rgb.astype(np.float64)) if scale is None else scale)
    err = np.abs(total - rgb.astype(np.float64))
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"sum {what}: worst |sum of passes - frame| / bound = {worst:.3g}, largest relative error {float((err / np.maximum(np.abs(rgb), 1e-30)).max()):.3g}")
    assert (err <= bound).all(), (what, worst)


# ------------------------------------------------------------------------------------------------------------------ 1. anchor --

@pytest.mark.parametrize("estimator", list(ESTIMATORS))
@pytest.mark.parametrize("scene", list(SCENES))
def test_the_frame_and_every_counter_are_the_list_schedules(hip, monkeypatch, scene, estimator):
    build, params = SCENES[scene]
    hs, p = build(), params()
    on = render_with_passes(hip, hs, p, estimator)
    assert on[2].rays_inline == 0 and on[2].tail_launches == 0 and on[2].rays_primary == on[2].samples == W * H * SPP
    monkeypatch.setenv("JADE_FUSED", "0")
    monkeypatch.setenv("JADE_TAIL", "0")
    with hip.scene(hs) as sc:
        set_estimator(sc, estimator)
        off = sc.render(p)
        with pytest.raises(B.JadeError) as ei:
            sc.passes()
        assert ei.value.code == _abi.JADE_ERR_INVALID and "jade_scene_set_passes" in str(ei.value)
    assert same_bits(on[0], off[0]) and np.array_equal(on[1], off[1])
    assert all_counters(on[2]) == all_counters(off[2])
    check_sum(on[0], on[3], SPP, what=f"{scene}/{estimator}")
    assert sum(bool(v.any()) for v in on[3].values()) >= 8, "most passes are lit on these scenes"


def test_set_and_unset_leaves_the_default_render(hip):
    build, params = SCENES["base"]
    hs, p = build(), params()
    with hip.scene(hs) as sc:
        assert not sc.passes_enabled
        first = sc.render(p)
        plain_bytes, rpp = sc.query(_abi.Q_STATE_BYTES), sc.query(_abi.Q_RECORDS_PER_PIXEL)
        sc.set_passes(True)
        on = sc.render(p)
        sc.passes()
        # the planes are the render's state - 424 B per record - and a render that keeps none gives them back
        records = 256 * (-(-W // 16)) * (-(-H // 16)) * rpp
        assert sc.query(_abi.Q_RECORDS_PER_PIXEL) == rpp and sc.query(_abi.Q_STATE_BYTES) == plain_bytes + 424 * records
        sc.set_passes(False)
        assert not sc.passes_enabled
        again = sc.render(p)
        assert sc.query(_abi.Q_STATE_BYTES) == plain_bytes
        with pytest.raises(B.JadeError):
            sc.passes()
    assert first[2].rays_inline > 0, "the default render runs the fused first pass"
    assert same_bits(first[0], again[0]) and np.array_equal(first[1], again[1]) and all_counters(first[2]) == all_counters(again[2])
    assert same_bits(first[0], on[0]) and np.array_equal(first[1], on[1])


# --------------------------------------------------------------------------------------------------------------------- 2. sum --

@pytest.mark.parametrize("env", [_abi.ENV_IMPORTANCE, _abi.ENV_MIXTURE])
@pytest.mark.parametrize("estimator", list(ESTIMATORS))
def test_the_passes_sum_to_the_frame_under_the_other_environment_samplings(hip, estimator, env):
    build, params = SCENES["lamp"]
    rgb, _, st, passes = render_with_passes(hip, build(), params(env_sampling=env), estimator)
    check_sum(rgb, passes, SPP, what=f"lamp/{estimator}/env {env}")


# --------------------------------------------------------------------------------------------------- 3. the float64 statement --

@pytest.mark.parametrize("name", list(PS.CASES))
def test_the_split_is_the_float64_statements(hip, name):
    e = PS.expected(name)
    frames = {}
    with hip.scene(e["hs"]) as sc:
        set_estimator(sc, PS.CASES[name].get("estimator", "reference"))
        sc.set_passes(True)

        def render(hs, p):
            rgb, _, _ = sc.render(p, want_bgr8=False)
            frames[p.frame] = (rgb, sc.passes())
            return frames[p.frame]

        PS.compare(render, name)
    # ... and check 2 with the bound as derived: the statement's own sum of |addend| per sample
    for f, frame in enumerate(PS.CASES[name]["frames"]):
        rgb, passes = frames[frame]
        keep = ~e["left_out"][f]
        scale = np.where(keep[..., None], e["absolute"][f], np.inf)
        check_sum(rgb, passes, 1, scale=np.maximum(scale, np.abs(rgb)), what=f"{name} frame {frame}")


# ------------------------------------------------------------------------------------------------------------------- 4. seams --

class _Scene:
    """A scene handle whose frames carry the 15 pass images under the frame: [16 H, W, 3]."""

    def __init__(self, sc):
        self._sc = sc
        self._on = False   # what the render in progress began with

    def __getattr__(self, name):
        return getattr(self._sc, name)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self._sc.close()

    def _under(self, rgb):
        return np.concatenate([rgb] + list(self._sc.passes().values()), axis=0) if self._on else rgb

    def render(self, p, **kw):
        self._on = self._sc.passes_enabled
        rgb, bgr, st = self._sc.render(p, **kw)
        return self._under(rgb), bgr, st

    def begin(self, p):
        self._on = self._sc.passes_enabled
        self._sc.begin(p)

    def resolve(self, *a, **kw):
        rgb, bgr = self._sc.resolve(*a, **kw)
        return self._under(rgb), bgr


class _Backend:
    def __init__(self, be):
        self._be = be

    def __getattr__(self, name):
        return getattr(self._be, name)

    def scene(self, hs, *a, **kw):
        return _Scene(self._be.scene(hs, *a, **kw))


def _case(name, estimator, cli_flags):
    def apply(sc):
        set_estimator(sc, estimator)
        sc.set_passes(True)

    # a camera mode is refused by the first check that applies: the cosine bounce's own where the estimator has one, else the passes'
    first = ("JADE_BOUNCE_COSINE",) if ESTIMATORS[estimator][0] == COS else ("passes", "jade_scene_set_passes")
    usable = [("do", apply), ("do", lambda sc: sc.set_lens(0.05, 4.0)), ("refused", "begin", first + ("lens",)),
              ("do", lambda sc: (sc.set_lens(0.0), sc.set_shutter(*MS._lamp_pose()))), ("refused", "render", first + ("shutter",)),
              ("do", lambda sc: (sc.set_shutter(None), sc.set_light_sampling(MS.ONE))), ("refused", "begin", ("passes", "JADE_LIGHTS_ONE")),
              ("do", lambda sc: sc.set_light_sampling(MS.ALL)), ("reference",),
              # ... and without passes the handle renders what its estimator allows: a lens, unless the cosine bounce refuses it
              ("do", lambda sc: (sc.set_passes(False), None if ESTIMATORS[estimator][0] == COS else sc.set_lens(0.05, 4.0))), ("finite",)]
    return MS.Case(name=name, scene=lambda: lamp_scenes.lamp_scene("lamp"), params=lamp_scenes.params, apply=apply,
                   switch=lambda sc: sc.set_passes(False), steps=(3, 2), shares=2, invariants=MS.camera_invariants,
                   small_scene=lambda: lamp_scenes.lamp_scene("lamp1"),
                   oracle_calls=lambda so: (lambda: so.set_passes(True), lambda: so.passes_enabled),
                   multi_unequal=[], multi_words="passes", usable=usable,
                   cli=dict(flags=cli_flags, suffix="light passes kept",
                            refused=[(["--passes", "x"] + MS._ON_THE_ORACLE, ("--passes needs the HIP backend",))]))


CASES = {c.name: c for c in (_case("passes", "reference", ["--passes", "p"]),
                             _case("passes+MIS", "MIS", ["--bounce", "cosine", "--direct", "mis", "--passes", "p"]))}
BITWISE_SCHEDULES = [env for env in MS.COMMON_SCHEDULES if "JADE_RECORDS_PER_PIXEL" not in env]


@pytest.fixture(scope="module")
def be(hip):
    return _Backend(hip)


@pytest.fixture
def ref(be, case):
    out = MS.reference(be, CASES[case])
    assert out[0].shape == (16 * lamp_scenes.HH, lamp_scenes.W, 3)
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_the_same_bits_and_counters_twice(be, ref, case):
    MS.check_twice(be, CASES[case], ref)


@pytest.mark.parametrize("case", list(CASES))
def test_the_same_bits_under_the_three_walks(be, ref, case):
    MS.check_walks(be, CASES[case], ref)


@pytest.mark.parametrize("case", list(CASES))
def test_steps_and_a_flush_equal_one_call(be, ref, case):
    MS.check_steps(be, CASES[case], ref)


@pytest.mark.parametrize("case", list(CASES))
def test_tile_shares_assemble_to_the_frame(be, ref, case):
    MS.check_shares(be, CASES[case], ref)


@pytest.mark.parametrize("env", BITWISE_SCHEDULES, ids=MS.schedule_id)
@pytest.mark.parametrize("case", list(CASES))
def test_schedules_are_one_result(be, ref, monkeypatch, case, env):
    MS.check_schedule(be, CASES[case], ref, env, monkeypatch.setenv)


@pytest.mark.parametrize("rpp", [1, 8])
@pytest.mark.parametrize("case", list(CASES))
def test_records_per_pixel_change_only_the_order_of_the_last_sum(be, ref, monkeypatch, case, rpp):
    c = CASES[case]
    p = c.params()
    monkeypatch.setenv("JADE_RECORDS_PER_PIXEL", str(rpp))
    with be.scene(c.scene()) as sc:
        c.apply(sc)
        sc.begin(p)
        assert sc.query(_abi.Q_RECORDS_PER_PIXEL) == rpp
        out = sc.render(p)
    h = p.height
    assert same_bits(out[0][:h], ref[0][:h]) and np.array_equal(out[1], ref[1]), "the frame, bit for bit"
    assert MS.counters(out[2]) == MS.counters(ref[2])
    frame = np.abs(ref[0][:h].astype(np.float64))
    bound = 2 * addends(p.spp) * U * frame
    for i, n in enumerate(NAMES):
        a, b = (v[(i + 1) * h:(i + 2) * h].astype(np.float64) for v in (out[0], ref[0]))
        assert (np.abs(a - b) <= bound).all(), (n, float(np.abs(a - b).max()))


@pytest.mark.parametrize("case", list(CASES))
def test_the_oracle_has_no_such_entry_point(oracle, case):
    MS.check_oracle_refuses(oracle, CASES[case])


@pytest.mark.parametrize("case", list(CASES))
def test_a_refusal_leaves_the_handle_usable(be, ref, case):
    MS.check_refusal_leaves_the_handle_usable(be, CASES[case], ref)


def test_pixel_rotation_is_refused_by_name(hip, monkeypatch):
    monkeypatch.setenv("JADE_PIXEL_ROTATE", "1")
    with hip.scene(lamp_scenes.lamp_scene("lamp1")) as sc:
        sc.set_passes(True)
        MS.refused(lambda: sc.begin(lamp_scenes.params()), _abi.JADE_ERR_UNSUPPORTED, ("passes", "JADE_PIXEL_ROTATE"))
        sc.set_passes(False)
        assert np.isfinite(sc.render(lamp_scenes.params())[0]).all()


def test_render_multi_refuses_a_handle_that_keeps_passes(hip):
    hs, p = lamp_scenes.lamp_scene("lamp"), lamp_scenes.params()
    with hip.scene(hs) as sc:
        plain = B.render_multi(hip, [sc], p)
        sc.set_passes(True)
        MS.refused(lambda: B.render_multi(hip, [sc], p), _abi.JADE_ERR_UNSUPPORTED, ("passes", "jade_scene_set_passes", "jade_render_passes"))
        sc.set_passes(False)
        again = B.render_multi(hip, [sc], p)
    assert same_bits(plain[0], again[0]) and np.array_equal(plain[1], again[1])


@pytest.mark.parametrize("case", list(CASES))
def test_the_command_line(case, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    MS.check_command_line(CASES[case], tmp_path)
    # ... and the 15 files beside the frame add up to it
    flags = [f if f != "p" else str(tmp_path / "q") for f in CASES[case].cli["flags"]]
    r = subprocess.run([CLI] + MS._CLI_BASE + flags + ["--out", str(tmp_path / "frame.pfm")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    frame = read_pfm(tmp_path / "frame.pfm")
    passes = {n: read_pfm(tmp_path / f"q.{n}.pfm") for n in NAMES}
    assert all(f"q.{n}.pfm" in r.stdout for n in NAMES)
    check_sum(frame, passes, 4, what="command line")
    assert sum(bool(v.any()) for v in passes.values()) >= 3


# ------------------------------------------------------------------------------------------------------------------ 5. on top --

def test_the_sum_holds_after_adaptive_sampling(hip):
    hs = lamp_scenes.lamp_scene("lamp")
    p = lamp_scenes.params(spp=64, w=W, h=H)
    with hip.scene(hs) as sc:
        sc.set_passes(True)
        rgb, _, tile_spp, _ = sc.render_adaptive(p, 4, 0.25)
        passes = sc.passes()
    counts = sorted(set(tile_spp.ravel().tolist()))
    print("tile sample counts:", counts)
    assert len(counts) > 1, "tiles stop at different counts"
    check_sum(rgb, passes, p.spp, what="adaptive")


def test_passes_between_steps_are_those_of_a_render_that_ended_there(hip):
    hs, p = lamp_scenes.lamp_scene("lamp"), lamp_scenes.params(spp=SPP, w=W, h=H)
    with hip.scene(hs) as sc:
        sc.set_passes(True)
        sc.begin(p)
        sc.step(3)
        mid = stacked(sc.passes())
        mid_rgb = sc.resolve()[0]
        sc.step(3)
        end, end_rgb = stacked(sc.passes()), sc.resolve()[0]
        sc.begin(p)
        sc.step(3)
        sc.flush()
        rgb3, three = sc.resolve()[0], stacked(sc.passes())
        whole = sc.render(p)
        all6 = stacked(sc.passes())
    assert same_bits(mid, three) and same_bits(mid_rgb, rgb3)
    assert same_bits(end, all6) and same_bits(end_rgb, whole[0])
    assert not same_bits(mid, end)
    check_sum(mid_rgb, dict(zip(NAMES, mid)), 3, what="after 3 of 6 samples")


def test_the_denoiser_exposure_and_glare_leave_the_passes_alone(hip):
    hs, p = lamp_scenes.lamp_scene("lamp"), lamp_scenes.params(spp=SPP, w=W, h=H)
    with hip.scene(hs) as sc:
        sc.set_passes(True)
        rgb, _, _ = sc.render(p)
        before = stacked(sc.passes())
        sc.denoise()
        sc.guides()
        sc.resolve(exposure="auto")
        sc.meter()
        sc.glare()
        after = stacked(sc.passes())
        rgb2 = sc.resolve()[0]
    assert same_bits(before, after) and same_bits(rgb, rgb2)
