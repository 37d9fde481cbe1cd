"""The seams of smooth shading on the device (include/jade_bvh.h, jade_scene_set_vertex_normals): a table that is flat everywhere and a
table that is cleared are today's render bit for bit; the smooth render twice, under the three walks, in steps, in tile shares and through
jade_render_multi is one result (the checks of tests/mode_seams.py on a case of its own); the refusals carry their texts; the command
line's --smooth is the API's frame; adaptive sampling, the denoiser, exposure and glare run on top."""
import subprocess

import numpy as np
import pytest

import mode_seams as MS
import smooth_cases as SC
import spec_scenes as SP
from conftest import B, counters
from jaderaytracerendering_amd import _abi, host as H
from render_helpers import CLI, all_counters, read_pfm, same_bits

pytestmark = pytest.mark.gpu
SIZE, SPP = 32, 8


def scene():
    return SC.ball(SP.JADE)


def params(**kw):
    eye, cam = H.camera_orbit(2.8, 20.0, 10.0)
    return B.make_params(SIZE, SIZE, SPP, eye, cam, frame=3, **kw)


def list_schedule(st):
    """No fused first pass (every camera ray goes through k_trace) and no tail kernel."""
    assert st.rays_inline == 0 and st.tail_launches == 0 and st.rays_tail == 0 and st.rays_primary == st.samples, all_counters(st)


def _multi_unequal(s1):
    s1.set_vertex_normals(None)


CASE = MS.Case(name="smooth", scene=scene, params=params, apply=lambda sc: None,       # Backend.scene() put the host scene's table on the handle
               switch=lambda sc: sc.set_vertex_normals(None), steps=(2, 4), shares=2, invariants=list_schedule, small_scene=lambda: SP.build("jade_cube"),   # (no table: the oracle cannot take one)
               oracle_calls=lambda so: (lambda: so.set_vertex_normals(None), lambda: so.vertex_normals_set()),
               multi_unequal=[_multi_unequal], multi_words="vertex normals")


@pytest.fixture(scope="module")
def ref(hip):
    out = MS.reference(hip, CASE)
    assert out[2].samples == SIZE * SIZE * SPP
    return out


def test_a_flat_table_is_the_parents_render_bit_for_bit(hip, monkeypatch):
    hs = scene()
    vn = hs.vertex_normals
    hs.vertex_normals = None
    t = hs.tri_f32()
    flat = np.repeat(t[:, None, 10:13], 3, 1).copy()
    p = params()
    for env in ({"JADE_FUSED": "0", "JADE_TAIL": "0"}, {}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        with hip.scene(hs) as sc:
            parent = sc.render(p)
            sc.set_vertex_normals(flat)
            assert sc.vertex_normals_set()
            out = sc.render(p)
            assert same_bits(out[0], parent[0]) and np.array_equal(out[1], parent[1]) and all_counters(out[2]) == all_counters(parent[2]), env
            # ... and clearing a table that is not flat gives the same render again
            sc.set_vertex_normals(vn)
            smooth = sc.render(p)
            assert not same_bits(smooth[0], parent[0])
            list_schedule(smooth[2])
            sc.set_vertex_normals(None)
            assert not sc.vertex_normals_set()
            back = sc.render(p)
            assert same_bits(back[0], parent[0]) and np.array_equal(back[1], parent[1]) and all_counters(back[2]) == all_counters(parent[2]), env
        for k in env:
            monkeypatch.delenv(k)
    assert parent[2].rays_inline > 0, "the default schedule has its fused first pass back"


def test_the_same_bits_and_counters_twice(hip, ref):
    MS.check_twice(hip, CASE, ref)


def test_the_same_bits_under_the_three_walks(hip, ref):
    MS.check_walks(hip, CASE, ref)


def test_steps_and_a_flush_equal_one_call_and_keep_the_table_they_began_with(hip, ref):
    MS.check_steps(hip, CASE, ref)


def test_tile_shares_assemble_to_the_frame(hip, ref):
    MS.check_shares(hip, CASE, ref)


def test_render_multi_on_one_device(hip, ref):
    MS.check_render_multi(hip, CASE, ref)


def test_the_oracle_has_no_such_entry_point(oracle):
    MS.check_oracle_refuses(oracle, CASE)


def test_a_wrong_count_is_invalid_and_non_finite_entries_are_taken(hip):
    hs = scene()
    with hip.scene(hs) as sc:
        MS.refused(lambda: sc.set_vertex_normals(hs.vertex_normals[:-1]), _abi.JADE_ERR_INVALID, ("triangle count",))
        assert sc.vertex_normals_set(), "the refused call left the table"
        vn = hs.vertex_normals.copy()
        vn[::3, 1] = np.nan
        vn[1::7, 2] = np.inf
        vn[2::5] = 0
        sc.set_vertex_normals(vn)
        rgb, _, st = sc.render(params())
        assert np.isfinite(rgb).all() and st.samples == SIZE * SIZE * SPP


REFUSALS = [
    ("shutter", lambda sc: sc.set_shutter(*H.camera_orbit(2.8, 20.0, 14.0)), ("smooth shading", "a shutter (jade_scene_set_shutter)")),
    ("one-light", lambda sc: sc.set_light_sampling(_abi.LIGHTS_ONE), ("smooth shading", "JADE_LIGHTS_ONE")),
    ("MIS", lambda sc: (sc.set_bounce_sampling(_abi.BOUNCE_COSINE), sc.set_direct_sampling(_abi.DIRECT_MIS)), ("smooth shading", "JADE_DIRECT_MIS")),
    ("passes", lambda sc: sc.set_passes(True), ("smooth shading", "passes (jade_scene_set_passes)")),
    ("branch", lambda sc: sc.set_branch_sampling(_abi.BRANCH_STRATIFIED), ("smooth shading", "JADE_BRANCH_STRATIFIED")),
    ("cosine+lens", lambda sc: (sc.set_bounce_sampling(_abi.BOUNCE_COSINE), sc.set_lens(0.05, 2.5)), ("bounce sampling: JADE_BOUNCE_COSINE", "lens")),
]


@pytest.mark.parametrize("name", [r[0] for r in REFUSALS])
def test_the_refusals_carry_their_texts_and_leave_the_handle_usable(hip, ref, name):
    _, put, words = next(r for r in REFUSALS if r[0] == name)
    with hip.scene(scene()) as sc:
        put(sc)
        MS.refused(lambda: sc.begin(params()), _abi.JADE_ERR_UNSUPPORTED, words)
        sc.set_vertex_normals(None)
        if words[0] == "smooth shading":       # without the table the same settings render
            assert np.isfinite(sc.render(params())[0]).all()
        else:                                  # somebody else's refusal: the same words with the table and without
            MS.refused(lambda: sc.begin(params()), _abi.JADE_ERR_UNSUPPORTED, words)
    with hip.scene(scene()) as sc:             # ... and a fresh handle with the table alone is the reference
        MS.is_reference(CASE, sc.render(params()), ref, name)


def test_the_accepted_rows_render(hip, ref):
    sky = SC.ball(SP.JADE, sky=True)
    for env_sampling in (_abi.ENV_REFERENCE, _abi.ENV_IMPORTANCE, _abi.ENV_MIXTURE):
        for put in (lambda sc: None, lambda sc: sc.set_bounce_sampling(_abi.BOUNCE_COSINE), lambda sc: sc.set_lens(0.05, 2.5)):
            with hip.scene(sky) as sc:
                put(sc)
                rgb, _, st = sc.render(params(env_sampling=env_sampling))
                assert np.isfinite(rgb).all() and rgb.max() > 0
                list_schedule(st)


def test_the_command_lines_smooth_frame_is_the_apis(hip, tmp_path):
    size, spp = 32, 4
    common = [CLI, "--config", "tiny", "--width", str(size), "--height", str(size), "--spp", str(spp)]
    r = subprocess.run(common + ["--smooth", "--out", "s.pfm"], capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    assert any(ln.startswith("Start...") and "smooth shading" in ln for ln in r.stdout.splitlines()), r.stdout
    r45 = subprocess.run(common + ["--smooth", "45", "--out", "s45.pfm"], capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert r45.returncode == 0, r45.stderr
    b = H.SceneBuilder()
    try:
        b.set_smoothing(60.0)
        cfg = b.config("tiny")
        hs = b.build()
    finally:
        b.close()
    assert hs.vertex_normals is not None
    p = B.params_from_config(cfg, spp=spp, walk=_abi.WALK_EARLY_EXIT)
    p.width = p.height = size
    with hip.scene(hs) as sc:
        rgb, _, _ = sc.render(p, want_bgr8=False)
        sc.set_vertex_normals(None)
        flat, _, _ = sc.render(p, want_bgr8=False)
    assert same_bits(read_pfm(tmp_path / "s.pfm"), rgb)
    assert not same_bits(rgb, flat), "the configuration has something to smooth"
    bad = subprocess.run(common + ["--smooth", "400", "--out", "x.pfm"], capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert bad.returncode == 2 and "--smooth takes an angle" in bad.stderr
    from conftest import ORACLE_LIB
    orc = subprocess.run(common + ["--smooth", "--backend", ORACLE_LIB, "--out", "x.pfm"], capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert orc.returncode == 2 and "--smooth needs the HIP backend" in orc.stderr


def test_adaptive_the_denoiser_exposure_and_glare_run_on_a_smooth_render(hip, ref):
    p = params()
    with hip.scene(scene()) as sc:
        rgb, _, tile_spp, st = sc.render_adaptive(p, 2, 0.05)
        assert np.isfinite(rgb).all() and (tile_spp > 0).all() and st.rays_inline == 0
        out = sc.render(p)
        MS.is_reference(CASE, out, ref, "after an adaptive render")
        dn, _ = sc.denoise()
        assert np.isfinite(dn).all() and not same_bits(dn, out[0])
        _, bgr, e, meter = sc.resolve(exposure="auto")
        assert e > 0 and meter.total == SIZE * SIZE and bgr.max() > 0
        gl, _, _ = sc.glare()
        assert np.isfinite(gl).all()
        again = sc.render(p)
        MS.is_reference(CASE, again, ref, "the passes on top leave the render alone")
