"""The seams of albedo textures on the device (include/jade_bvh.h, "The surface colour, stated"; jade_scene_set_textures).  A texture
multiplies radiance and nothing else, which gives identities that hold bit for bit: an image of ones is the untextured render, a constant
image the render with the constant baked into the materials, a block atlas the render baked triangle by triangle, and any image leaves
every counter of jade_stats where it was.  Then the checks of tests/mode_seams.py on a case of its own (twice, the walks, steps, shares,
jade_render_multi, the oracle's refusal), the refusals and their texts, the arguments that are JADE_ERR_INVALID, and what runs on top.

A textured render runs the list schedule (no fused first pass, no k_tail): its frame is the default schedule's in every bit, its counters
are compared in full with the untextured render under JADE_FUSED=0 JADE_TAIL=0 and in conftest.counters' keys with the default one."""
import subprocess

import numpy as np
import pytest

import mode_seams as MS
import smooth_cases as SC
import spec_scenes as SP
import texture_cases as TC
from conftest import B, counters
from jaderaytracerendering_amd import _abi, host as H
from render_helpers import CLI, all_counters, read_pfm, same_bits

pytestmark = pytest.mark.gpu
F32 = np.float32
SIZE, SPP = 32, 8
LIST_SCHEDULE = {"JADE_FUSED": "0", "JADE_TAIL": "0"}


def ball(normals, sky=True):
    """tests/smooth_cases.py's jade ball over the floor under the light and the 8 x 4 sky, with its vertex normals or without."""
    hs = SC.ball(SP.JADE, sky=sky)
    if not normals:
        hs.vertex_normals = None
    return hs


def params(**kw):
    eye, cam = H.camera_orbit(2.8, 20.0, 10.0)
    return B.make_params(SIZE, SIZE, SPP, eye, cam, frame=3, **kw)


def list_schedule(st):
    assert st.rays_inline == 0 and st.tail_launches == 0 and st.rays_tail == 0 and st.rays_primary == st.samples, all_counters(st)


def same_render(a, b, what, full=True):
    assert same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]), what
    assert (all_counters(a[2]) == all_counters(b[2])) if full else (counters(a[2]) == counters(b[2])), (what, all_counters(a[2]), all_counters(b[2]))


def ones(hs):
    return ([np.ones((4, 4, 3), F32)], TC.planar_uv(hs), np.zeros(hs.n_triangles, np.int32))


MODES = {
    "reference": lambda sc: None,
    "cosine": lambda sc: sc.set_bounce_sampling(_abi.BOUNCE_COSINE),
    "lens": lambda sc: sc.set_lens(0.05, 2.5),
}


# ------------------------------------------------------------------------------------------------------------------ identities --
@pytest.mark.parametrize("normals", (False, True), ids=("flat", "vertex-normals"))
@pytest.mark.parametrize("mode", sorted(MODES))
def test_an_image_of_ones_is_the_untextured_render(hip, monkeypatch, normals, mode):
    hs = ball(normals)
    for env in (LIST_SCHEDULE, {}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        with hip.scene(hs) as sc:
            MODES[mode](sc)
            for env_sampling in (_abi.ENV_REFERENCE, _abi.ENV_IMPORTANCE, _abi.ENV_MIXTURE):
                p = params(env_sampling=env_sampling)
                sc.set_textures(None)
                plain = sc.render(p)
                sc.set_textures(*ones(hs))
                assert sc.textures
                out = sc.render(p)
                list_schedule(out[2])
                same_render(out, plain, (mode, env_sampling, env), full=bool(env) or mode == "lens" or normals)
        for k in env:
            monkeypatch.delenv(k)
    assert (plain[2].rays_inline > 0) == (mode != "lens" and not normals), "the default schedule has its fused first pass back"


def test_a_cleared_table_and_a_table_naming_no_image_are_no_table(hip):
    hs = ball(False)
    p = params()
    with hip.scene(hs) as sc:
        plain = sc.render(p)
        assert plain[2].rays_inline > 0 and not sc.textures
        images, uv, image_of = ones(hs)
        sc.set_textures([TC.random_image()], uv, np.full(hs.n_triangles, -1, np.int32))
        assert sc.textures
        same_render(sc.render(p), plain, "a table naming no image")
        sc.set_textures([TC.random_image()], uv, image_of)
        assert not same_bits(sc.render(p)[0], plain[0])
        sc.set_textures(None)
        assert not sc.textures
        same_render(sc.render(p), plain, "a cleared table")
        sc.set_textures([], uv, image_of)
        assert not sc.textures


@pytest.mark.parametrize("normals", (False, True), ids=("flat", "vertex-normals"))
def test_a_constant_image_is_the_scene_with_the_constant_baked_in(hip, normals):
    hs = ball(normals)
    c = np.array([0.3, 1.7, 0.625], F32)                               # (above 1 passes through)
    tex = ([np.ones((4, 4, 3), F32), np.broadcast_to(c, (5, 7, 3)).copy()], TC.planar_uv(hs), np.ones(hs.n_triangles, np.int32))
    for mode in sorted(MODES):
        for env_sampling in (_abi.ENV_REFERENCE, _abi.ENV_IMPORTANCE):
            p = params(env_sampling=env_sampling)
            with hip.scene(hs) as sc:
                MODES[mode](sc)
                sc.set_textures(*tex)
                out = sc.render(p)
            with hip.scene(TC.baked(hs, c)) as sb:
                MODES[mode](sb)
                same_render(out, sb.render(p), (mode, env_sampling), full=False)


def atlas(hs, seed=21):
    """Two block atlases of different sizes - 16 x 16 in 4 x 4 blocks and 32 x 8 (W x H) in 8 x 2 blocks, every block 4 x 4 texels of one
    colour - dealt over the triangles: each triangle gets a block and corner UVs at least one texel inside it (shifted by whole
    periods), so that every tap of every point of the triangle reads the block's colour.  Returns (textures, colour per triangle)."""
    rng = np.random.default_rng(seed)
    n = hs.n_triangles
    images, blocks = [], []
    for Hh, W in ((16, 16), (8, 32)):
        cols = rng.uniform(0.1, 1.6, (Hh // 4, W // 4, 3)).astype(F32)
        images.append(np.repeat(np.repeat(cols, 4, 0), 4, 1))
        blocks.append(cols)
    image_of = rng.integers(0, 2, n).astype(np.int32)
    uv = np.zeros((n, 3, 2), F32)
    colour = np.zeros((n, 3), F32)
    for t in range(n):
        cols = blocks[image_of[t]]
        Hh, W = images[image_of[t]].shape[:2]
        bj, bi = rng.integers(0, cols.shape[0]), rng.integers(0, cols.shape[1])
        u = (4 * bi + rng.uniform(1.0, 3.0, 3)) / W + rng.integers(-2, 3)
        v = (4 * bj + rng.uniform(1.0, 3.0, 3)) / Hh + rng.integers(-2, 3)
        uv[t] = np.stack([u, v], 1)
        colour[t] = cols[bj, bi]
    return (images, uv, image_of), colour


@pytest.mark.parametrize("normals", (False, True), ids=("flat", "vertex-normals"))
def test_a_block_atlas_is_the_scene_baked_triangle_by_triangle(hip, normals):
    hs = ball(normals)
    tex, colour = atlas(hs)
    p = params()
    with hip.scene(hs) as sc:
        sc.set_textures(*tex)
        out = sc.render(p)
    with hip.scene(TC.baked(hs, colour)) as sb:
        flat = sb.render(p)
    same_render(out, flat, "atlas", full=False)
    assert len({tuple(c) for c in colour}) > 8


def test_a_random_image_leaves_every_counter_where_it_was(hip, monkeypatch):
    for k, v in LIST_SCHEDULE.items():
        monkeypatch.setenv(k, v)
    for normals in (False, True):
        hs = ball(normals)
        with hip.scene(hs) as sc:
            for mode in sorted(MODES):
                sc.set_bounce_sampling(_abi.BOUNCE_UNIFORM)
                sc.set_lens(None)
                MODES[mode](sc)
                p = params(env_sampling=_abi.ENV_MIXTURE if mode == "reference" else _abi.ENV_REFERENCE)
                sc.set_textures(None)
                plain = sc.render(p)
                sc.set_textures([TC.random_image(), TC.random_image(13, 32)], TC.planar_uv(hs), np.arange(hs.n_triangles) % 3 - 1)
                out = sc.render(p)
                assert all_counters(out[2]) == all_counters(plain[2]), (normals, mode)
                assert not same_bits(out[0], plain[0]) and np.isfinite(out[0]).all()


# ------------------------------------------------------------------------------------------------- the checks of tests/mode_seams.py --
def scene():
    return TC.textured(ball(True), [TC.random_image()])


CASE = MS.Case(name="textures", scene=scene, params=params, apply=lambda sc: None,         # Backend.scene() put the host scene's table on the handle
               switch=lambda sc: sc.set_textures(None), steps=(2, 4), shares=2, invariants=list_schedule, small_scene=lambda: SP.build("jade_cube"),
               oracle_calls=lambda so: (lambda: so.set_textures(None), lambda: so.textures),
               multi_unequal=[lambda s1: s1.set_textures(None)], multi_words="textures")


@pytest.fixture(scope="module")
def ref(hip):
    out = MS.reference(hip, CASE)
    assert out[2].samples == SIZE * SIZE * SPP
    return out


def test_the_same_bits_and_counters_twice(hip, ref):
    MS.check_twice(hip, CASE, ref)


def test_the_same_bits_under_the_three_walks(hip, ref):
    MS.check_walks(hip, CASE, ref)


def test_steps_and_a_flush_equal_one_call_and_keep_the_table_they_began_with(hip, ref):
    MS.check_steps(hip, CASE, ref)


def test_a_render_in_progress_keeps_its_tables_when_vertex_normals_arrive(hip):
    """A textured render begun without vertex normals reads the all-flat table it began with, whatever the handle is given before the flush."""
    hs = TC.textured(ball(False), [TC.random_image()])
    vn = ball(True).vertex_normals
    p = params()
    with hip.scene(hs) as sc:
        want = sc.render(p)
        sc.begin(p)
        st = _abi.Stats()
        sc.step(4, st)
        sc.set_vertex_normals(vn)
        sc.set_textures(None)
        sc.step(4, st)
        sc.flush(st)
        rgb, bgr = sc.resolve()
        assert same_bits(rgb, want[0]) and counters(st) == counters(want[2])
        smooth = sc.render(p)                                          # the next render takes what the handle carries now
        assert not same_bits(smooth[0], want[0])


def test_tile_shares_assemble_to_the_frame(hip, ref):
    MS.check_shares(hip, CASE, ref)


def test_render_multi_on_one_device(hip, ref):
    MS.check_render_multi(hip, CASE, ref)


def test_the_oracle_has_no_such_entry_point(oracle):
    MS.check_oracle_refuses(oracle, CASE)


# ---------------------------------------------------------------------------------------------------------------------- refusals --
REFUSALS = [
    ("shutter", lambda sc: sc.set_shutter(*H.camera_orbit(2.8, 20.0, 14.0)), ("a shutter (jade_scene_set_shutter)",)),
    ("one-light", lambda sc: sc.set_light_sampling(_abi.LIGHTS_ONE), ("JADE_LIGHTS_ONE",)),
    ("MIS", lambda sc: (sc.set_bounce_sampling(_abi.BOUNCE_COSINE), sc.set_direct_sampling(_abi.DIRECT_MIS)), ("JADE_DIRECT_MIS",)),
    ("passes", lambda sc: sc.set_passes(True), ("passes (jade_scene_set_passes)",)),
    ("branch", lambda sc: sc.set_branch_sampling(_abi.BRANCH_STRATIFIED), ("JADE_BRANCH_STRATIFIED",)),
]


@pytest.mark.parametrize("name", [r[0] for r in REFUSALS])
def test_the_refusals_carry_their_texts_and_leave_the_handle_usable(hip, ref, name):
    _, put, words = next(r for r in REFUSALS if r[0] == name)
    hs = scene()
    with hip.scene(hs) as sc:
        put(sc)
        text = MS.refused(lambda: sc.begin(params()), _abi.JADE_ERR_UNSUPPORTED, words + ("smooth shading (jade_scene_set_vertex_normals) does not run",))
        sc.set_vertex_normals(None)                                    # the textures alone: the same words with their name for a subject
        alone = MS.refused(lambda: sc.begin(params()), _abi.JADE_ERR_UNSUPPORTED, words + ("textures (jade_scene_set_textures) do not run",))
        assert alone.split(" run ", 1)[1] == text.split(" run ", 1)[1]
        sc.set_textures(None)                                          # without either table the same settings render
        assert np.isfinite(sc.render(params())[0]).all()
    with hip.scene(hs) as sc:                                          # ... and a fresh handle with the tables alone is the reference
        MS.is_reference(CASE, sc.render(params()), ref, name)


def test_cosine_bounces_under_a_lens_keep_their_own_refusal(hip):
    with hip.scene(scene()) as sc:
        sc.set_bounce_sampling(_abi.BOUNCE_COSINE)
        sc.set_lens(0.05, 2.5)
        MS.refused(lambda: sc.begin(params()), _abi.JADE_ERR_UNSUPPORTED, ("bounce sampling: JADE_BOUNCE_COSINE", "lens"))


def test_the_arguments_that_are_invalid(hip, ref):
    hs = scene()
    images, uv, image_of = hs.textures
    n = hs.n_triangles
    with hip.scene(hs) as sc:
        bad = [
            (lambda: sc.set_textures(images, uv[:-1], image_of[:-1]), ("triangle count", str(n - 1))),
            (lambda: sc.set_textures(images, uv, np.where(np.arange(n) == 5, 1, image_of)), ("image_of[5] = 1",)),
            (lambda: sc.set_textures(images, uv, np.where(np.arange(n) == 7, -2, image_of)), ("image_of[7] = -2",)),
            (lambda: sc.set_textures(images + [np.zeros((0, 4, 3), F32)], uv, image_of), ("image 1 is 4 x 0",)),
            (lambda: sc.set_textures([np.zeros((1, 16385, 3), F32)], uv, image_of), ("image 0 is 16385 x 1",)),
            (lambda: sc.set_textures([np.ones((1, 1, 3), F32)] * 65537, uv, image_of), ("65537 images",)),
        ]
        for value in (np.nan, np.inf, -np.inf):
            im = images[0].copy()
            im[3, 5, 1] = value
            bad.append((lambda im=im: sc.set_textures([images[0], im], uv, image_of), ("image 1", "not finite", "(5, 3)")))
        for call, words in bad:
            MS.refused(call, _abi.JADE_ERR_INVALID, ("textures",) + words)
            assert sc.textures, "the refused call left the table"
        MS.is_reference(CASE, sc.render(params()), ref, "... as it was")
        # UVs that are not finite are taken: those vertices have c = (1, 1, 1); negative texels and texels above 1 pass through
        wild = uv.copy()
        wild[::3, 0, 0] = np.nan
        wild[1::5, 1, 1] = np.inf
        sc.set_textures([np.float32(2.5) * images[0] - np.float32(0.5)], wild, image_of)
        rgb, _, st = sc.render(params())
        assert st.samples == SIZE * SIZE * SPP and np.isfinite(rgb).all()
        assert counters(st) == counters(ref[2])


def test_the_accepted_rows_render(hip):
    for normals in (False, True):
        hs = TC.textured(ball(normals), [TC.random_image()])
        for env_sampling in (_abi.ENV_REFERENCE, _abi.ENV_IMPORTANCE, _abi.ENV_MIXTURE):
            for mode in sorted(MODES):
                with hip.scene(hs) as sc:
                    MODES[mode](sc)
                    rgb, _, st = sc.render(params(env_sampling=env_sampling))
                    assert np.isfinite(rgb).all() and rgb.max() > 0
                    list_schedule(st)


def test_the_command_lines_textured_frame_is_the_apis(hip, tmp_path):
    size, spp = 32, 4
    rng = np.random.default_rng(31)
    img = rng.integers(0, 256, (6, 10, 3)).astype(np.uint8)
    (tmp_path / "wall.ppm").write_bytes(b"P6\n10 6\n255\n" + img.tobytes())
    common = [CLI, "--config", "tiny", "--width", str(size), "--height", str(size), "--spp", str(spp)]
    flags = ["--texture", "0=checker:64:4", "--texture", "5=wall.ppm@planar-y"]
    r = subprocess.run(common + flags + ["--out", "t.pfm"], capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    assert any(ln.startswith("Start...") and ln.endswith(", textures") for ln in r.stdout.splitlines()), r.stdout
    b = H.SceneBuilder()
    try:
        b.set_object_texture(0, H.texture_checker(64, 4, (0.9, 0.9, 0.9), (0.15, 0.15, 0.15)))
        b.set_object_texture(5, H.load_texture(tmp_path / "wall.ppm"), H.UV_PLANAR_Y)
        cfg = b.config("tiny")
        hs = b.build()
    finally:
        b.close()
    assert hs.textures is not None and len(hs.textures[0]) == 2 and set(hs.textures[2].tolist()) == {-1, 0, 1}
    p = B.params_from_config(cfg, spp=spp, walk=_abi.WALK_EARLY_EXIT)
    p.width = p.height = size
    with hip.scene(hs) as sc:
        assert sc.textures
        rgb, _, _ = sc.render(p, want_bgr8=False)
        sc.set_textures(None)
        plain, _, _ = sc.render(p, want_bgr8=False)
    assert same_bits(read_pfm(tmp_path / "t.pfm"), rgb)
    assert not same_bits(rgb, plain), "the configuration shows its textures"
    for bad, code, words in ((["--texture", "checker"], 2, "K=IMAGE"), (["--texture", "99=checker"], 2, "objects 0 .. 5"),
                             (["--texture", "0=checker@sideways"], 2, "projection"), (["--texture", "0=none.ppm"], 1, "open failed"),
                             (["--texture", "0=checker", "--texture", "0=checker"], 2, "twice")):
        r = subprocess.run(common + bad + ["--out", "x.pfm"], capture_output=True, text=True, timeout=300, cwd=tmp_path)
        assert r.returncode == code and words in r.stderr, (bad, r.returncode, r.stderr)
    from conftest import ORACLE_LIB
    orc = subprocess.run(common + flags[:2] + ["--backend", ORACLE_LIB, "--out", "x.pfm"], capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert orc.returncode == 2 and "--texture needs the HIP backend" in orc.stderr


def test_adaptive_the_denoiser_exposure_and_glare_run_on_a_textured_render(hip, ref):
    p = params()
    with hip.scene(scene()) as sc:
        rgb, _, tile_spp, st = sc.render_adaptive(p, 2, 0.05)
        assert np.isfinite(rgb).all() and (tile_spp > 0).all() and st.rays_inline == 0
        out = sc.render(p)
        MS.is_reference(CASE, out, ref, "after an adaptive render")
        textured_albedo = sc.guides(4)["albedo"]
        dn, _ = sc.denoise()
        assert np.isfinite(dn).all() and not same_bits(dn, out[0])
        _, bgr, e, meter = sc.resolve(exposure="auto")
        assert e > 0 and meter.total == SIZE * SIZE and bgr.max() > 0
        gl, _, _ = sc.glare()
        assert np.isfinite(gl).all()
        again = sc.render(p)
        MS.is_reference(CASE, again, ref, "the passes on top leave the render alone")
        sc.set_textures(None)
        sc.render(p)
        assert not same_bits(sc.guides(4)["albedo"], textured_albedo), "the albedo guide carries the image"
