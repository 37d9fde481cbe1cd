"""The light passes without a device: the float64 statement (tests/passes_spec.py) regroups jade_spec.sample's colour and nothing else, the
reference's two quirks land where include/jade_bvh.h says, the cases the device is compared on reach all 15 passes, every check fails on a
wrong stand-in, and shade_mode_for (csrc/jade_runtime.h) accepts exactly the nine new modes beside the 27 old ones."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import jade_spec
import long_paths as LP
import passes_spec as PS
from conftest import ROOT
from jaderaytracerendering_amd import _abi

NAMES = PS.NAMES
IDX = {n: i for i, n in enumerate(NAMES)}


@pytest.fixture(scope="module")
def cases():
    return {name: PS.expected(name) for name in PS.CASES}


def _colours(name, e):
    """The estimator's own sample() (jade_spec, bounce_spec, mis_spec) of every sample of a case."""
    c = PS.CASES[name]
    spec = PS.spec_of(name)
    S = spec.Scene(e["hs"], 1 if c["env_sampling"] == PS.IMP else 0, 0)
    return np.array([[[spec.sample(S, x, y, PS.SIZE, PS.SIZE, e["eye"], e["cam"], frame) for x in range(PS.SIZE)] for y in range(PS.SIZE)]
                     for frame in c["frames"]])


def check_sum(passes, colour):
    """The passes of a sample add up to its colour within 1e-12 relative (of the sum of |pass|: the regrouping's own rounding)."""
    total = passes.sum(-2)
    scale = np.maximum(np.abs(passes).sum(-2), 1e-300)
    assert (np.abs(total - colour) <= 1e-12 * scale).all(), float((np.abs(total - colour) / scale).max())


@pytest.mark.parametrize("name", list(PS.CASES))
def test_the_passes_sum_to_the_sample(cases, name):
    e = cases[name]
    colour = _colours(name, e)
    check_sum(e["passes"], colour)
    wrong = e["passes"].copy()
    wrong[..., int(np.abs(wrong).sum((0, 1, 2, 4)).argmax()), :] = 0.0   # a stand-in that drops a class: the case's largest
    with pytest.raises(AssertionError):
        check_sum(wrong, colour)


def test_the_loop_that_keeps_the_stack_is_the_modules_own():
    """passes_spec.evaluate against bounce_spec.sample and mis_spec.sample: the same colour in every bit, the same trace."""
    for name in ("two_lamps_cosine", "patchwork_mis_importance"):
        c, spec = PS.CASES[name], PS.spec_of(name)
        e = PS.expected(name)
        S = spec.Scene(e["hs"], 1 if c["env_sampling"] == PS.IMP else 0, 0)
        for y in range(PS.SIZE):
            for x in range(0, PS.SIZE, 2):
                tr, tr2 = [], []
                want = spec.sample(S, x, y, PS.SIZE, PS.SIZE, e["eye"], e["cam"], c["frames"][0], tr)
                got = PS.evaluate(spec, S, x, y, PS.SIZE, PS.SIZE, e["eye"], e["cam"], c["frames"][0], tr2, {})
                assert np.array_equal(got, want) and tr2 == tr, (name, x, y)


def test_under_mis_the_bounce_term_and_the_weighted_terms_are_emitter_parts(cases):
    """A vertex whose indirect ray found a weighted emitter (mis-bounce-lit, mis-sss-bounce-lit) under a sky of zeros has T_B in its emitter
    part and nothing in its sky part; the MIS cases hold such samples and samples with w_L-weighted terms."""
    lit = weighted = 0
    for name in ("two_lamps_mis", "patchwork_mis_importance"):
        e = cases[name]
        emitter = [i for i, n in enumerate(NAMES) if "_emitter_" in n and not n.startswith("bssrdf")]
        for (f, y, x), tr in e["traces"].items():
            if e["left_out"][f, y, x]:
                continue
            if "mis-bounce-lit" in tr or "mis-sss-bounce-lit" in tr:
                assert e["passes"][f, y, x][emitter].any(), (name, f, x, y, tr)
                lit += 1
            weighted += "mis-weighted" in tr
    assert lit >= 3 and weighted >= 100, (lit, weighted)
    # ... and the split differs from cosine bounces' on the same scene and frames: in the emitter passes of diffuse and SSS-diffuse vertices
    a, b = cases["two_lamps_mis"]["passes"], cases["two_lamps_cosine"]["passes"]
    first = [i for i, n in enumerate(NAMES) if n in ("diffuse_emitter_first", "sss_emitter_first")]
    sky = [i for i, n in enumerate(NAMES) if n in ("diffuse_sky_first", "sss_sky_first", "background", "bssrdf_emitter_first")]
    assert not np.allclose(a[..., first, :], b[..., first, :], rtol=1e-6, atol=0) and np.allclose(a[..., sky, :], b[..., sky, :], rtol=1e-9, atol=1e-12)


def check_lit(cases):
    """compare() lets 2 % of a case's samples disagree in a pass: every pass must be lit in more than that share of the compared samples of
    some case, or a pass could be wrong wherever it is lit and still pass.  Returns {pass: the largest share}."""
    best = {}
    for name, e in cases.items():
        keep = ~e["left_out"]
        share = (e["passes"][keep] != 0).any(axis=2).mean(axis=0)
        for n, v in zip(NAMES, share):
            best[n] = max(best.get(n, 0.0), float(v))
    assert all(v > 0.02 for v in best.values()), {n: round(v, 4) for n, v in best.items() if v <= 0.02}
    return best


def test_every_pass_is_lit_in_more_samples_than_may_disagree(cases):
    print({n: round(v, 3) for n, v in check_lit(cases).items()})
    with pytest.raises(AssertionError):
        check_lit({"mirror_floor": cases["mirror_floor"]})


def check_open(passes, traces):
    """A refract-open sample keeps the camera vertex's emission and nothing else.  Returns how many there were."""
    n = 0
    for (f, y, x), tr in traces.items():
        if "refract-open" in tr:
            n += 1
            rest = np.delete(passes[f, y, x], PS.EMISSION, axis=0)
            assert not rest.any(), (f, x, y, tr)
    return n


def test_refract_open_samples_keep_only_the_camera_vertexs_emission(cases):
    e = cases["glass_cube"]
    assert check_open(e["passes"], e["traces"]) >= 1
    # ... among them one that had gathered something before the loop gave up (a push ahead of the refraction), or at least one glass-exit sky sample
    exits = [k for k, tr in e["traces"].items() if "refract" in tr and "refract-open" not in tr and e["passes"][k][PS.SPECULAR_SKY].any()]
    assert exits, "no glass-exit sky sample"
    wrong = e["passes"].copy()
    k = next(k for k, tr in e["traces"].items() if "refract-open" in tr)
    wrong[k][IDX["diffuse_emitter_later"]] = 1.0    # a stand-in that keeps what the sample had gathered
    with pytest.raises(AssertionError):
        check_open(wrong, e["traces"])


def check_cap(passes, stack, l_dir):
    """A path that ended by its 128th push in a closed diffuse room: the later diffuse passes hold every pushed vertex but the first and
    the last vertex's l_dir a second time, through every rate.  Returns that second addend."""
    assert len(stack) == LP.CAP and np.array_equal(stack[-1][0], l_dir) and l_dir.any()
    thr, later = np.ones(3), np.zeros(3)
    for i, (d, r) in enumerate(stack):
        if i:
            later = later + thr * d
        thr = thr * r
    second = thr * l_dir
    got = passes[IDX["diffuse_emitter_later"]] + passes[IDX["diffuse_sky_later"]]
    assert (np.abs(got - (later + second)) <= 1e-12 * np.abs(later + second)).all()
    assert (np.abs(second) > 1e-6 * np.abs(got)).any(), "the doubled term is a visible share of the pass"
    return second


def test_a_128_push_path_counts_its_last_vertex_twice_in_its_pass():
    name, r = next((n, r) for n, r in LP.recorded("cap", places=("alone",)) if n == "lit")
    S = jade_spec.Scene(LP.scene(name))
    eye, cam = LP.camera(name)
    tr, info = [], {}
    colour = jade_spec.sample(S, 0, 0, 1, 1, eye, cam, r["frame"], tr, info)
    assert info["pushes"] == LP.CAP
    passes = PS.split(S, 0, 0, 1, 1, eye, cam, r["frame"])
    check_sum(passes, colour)
    second = check_cap(passes, info["stack"], info["l_dir"])
    # a stand-in that counts the vertex once is short by the second addend: of the pass, and of the sample's colour
    wrong = passes.copy()
    wrong[IDX["diffuse_emitter_later"]] -= second
    with pytest.raises(AssertionError):
        check_cap(wrong, info["stack"], info["l_dir"])
    with pytest.raises(AssertionError):
        check_sum(wrong, colour)


def check_reach(cases):
    """Every one of the 15 passes is non-zero somewhere over the cases the device is compared on."""
    reached = np.zeros(len(NAMES), bool)
    for e in cases.values():
        keep = ~e["left_out"]
        reached |= (e["passes"][keep] != 0).any(axis=(0, 2))
    assert reached.all(), [n for n, r in zip(NAMES, reached) if not r]


def test_the_device_cases_reach_every_pass(cases):
    check_reach(cases)
    for name, e in cases.items():
        assert e["left_out"].sum() <= PS.MAX_LEFT_OUT * e["left_out"].size, name
    with pytest.raises(AssertionError):
        check_reach({k: v for k, v in cases.items() if k == "mirror_floor"} | {"x": dict(cases["mirror_floor"], passes=cases["mirror_floor"]["passes"] * 0)})


def test_negative_addends_come_from_schlick_out_alone(cases):
    """What check 2 of tests/test_gpu_passes.py scales its bound with: where every addend of a pixel is >= 0 the sum of |addend| is the
    colour; the reference's schlick_out (R0 - (1 - R0)(1 - cos)^5) is the one factor that can be negative, and it sits in the BSSRDF
    branch (its terms and its rate) and in the refraction loop (its rate): a sample that went through neither has no negative addend."""
    for name, e in cases.items():
        neg = (e["passes"] < 0).any(axis=(3, 4))
        for (f, y, x), tr in e["traces"].items():
            if neg[f, y, x]:
                assert "bssrdf" in tr or "refract" in tr, (name, f, x, y, tr)
        assert (e["absolute"] >= np.abs(e["passes"].sum(3)) * (1 - 1e-12)).all()


def test_the_comparison_fails_on_a_wrong_split(cases):
    """passes_spec.compare against a stand-in that renders the statement itself, then one that books the sky with the emitters."""
    name = "two_lamps"
    e = cases[name]

    def stand_in(wrong):
        def render(hs, p):
            f = PS.CASES[name]["frames"].index(p.frame)
            v = e["passes"][f].astype(np.float32).copy()
            if wrong:
                v[..., IDX["diffuse_emitter_first"], :] += v[..., IDX["diffuse_sky_first"], :]
                v[..., IDX["diffuse_sky_first"], :] = 0
            return v.sum(2), {n: v[:, :, i] for i, n in enumerate(NAMES)}
        return render

    PS.compare(stand_in(False), name)
    with pytest.raises(AssertionError):
        PS.compare(stand_in(True), name)


# ------------------------------------------------------------------------------------------------------------ shade_mode_for --
ENVIS, LENS, SHUTTER, LIGHTS, COSINE, MIS, ENVMIX, PASSES = (1 << i for i in range(8))
ENV_BITS = {_abi.ENV_REFERENCE: 0, _abi.ENV_IMPORTANCE: ENVIS, _abi.ENV_MIXTURE: ENVIS | ENVMIX}
ALL = list(itertools.product(ENV_BITS, (0, 1), (0, 1), (_abi.LIGHTS_ALL, _abi.LIGHTS_ONE), (_abi.BOUNCE_UNIFORM, _abi.BOUNCE_COSINE),
                             (_abi.DIRECT_RAYS, _abi.DIRECT_MIS)))


@pytest.fixture(scope="module")
def dbg():
    path = os.path.join(ROOT, "jaderaytracerendering_amd", "lib", "libjade_hip_debug.so")
    assert os.path.exists(path), "libjade_hip_debug.so missing: run `make hipvariants` (or __graft_entry__.build())"
    lib = C.CDLL(path)
    lib.jade_debug_shade_mode_env_host.restype = C.c_int
    lib.jade_debug_shade_mode_env_host.argtypes = [C.c_int32] * 6 + [C.POINTER(C.c_uint32)]
    lib.jade_debug_shade_mode_passes_host.restype = C.c_int
    lib.jade_debug_shade_mode_passes_host.argtypes = [C.c_int32] * 7 + [C.POINTER(C.c_uint32)]
    lib.jade_last_error.restype = C.c_char_p
    return lib


def _ask(dbg, combo, passes=None):
    mode = C.c_uint32(0xdeadbeef)
    rc = dbg.jade_debug_shade_mode_env_host(*combo, C.byref(mode)) if passes is None else dbg.jade_debug_shade_mode_passes_host(*combo, passes, C.byref(mode))
    return rc, mode.value, (dbg.jade_last_error() or b"").decode()


def test_exactly_the_nine_new_modes_are_accepted_beside_the_old_ones(dbg):
    assert len(ALL) == 96   # three environment samplings x 2^5 settings, each asked with passes off and on
    old, new = {}, {}
    for combo in ALL:
        before = _ask(dbg, combo)
        off = _ask(dbg, combo, 0)
        assert off[0] == before[0] and off[1] == before[1] and (off[0] == _abi.JADE_OK or off[2] == before[2]), ("passes off answers as before", combo)
        if before[0] == _abi.JADE_OK:
            old[combo] = before[1]
        rc, mode, text = _ask(dbg, combo, 1)
        env, lens, shutter, lights, bounce, direct = combo
        if rc == _abi.JADE_OK:
            new[combo] = mode
            assert mode == old[combo] | PASSES
        else:
            assert rc == _abi.JADE_ERR_UNSUPPORTED and mode == 0xdeadbeef
            if before[0] != _abi.JADE_OK:
                assert text == before[2], "the other modes' refusals come first and keep their texts"
            else:
                assert "passes" in text and "jade_scene_set_passes" in text
                assert ("lens" in text) if lens else ("shutter" in text) if shutter else ("JADE_LIGHTS_ONE" in text), text
    assert len(old) == 27 and len(new) == 9
    want = {(env, 0, 0, _abi.LIGHTS_ALL, b, d) for env in ENV_BITS
            for b, d in ((_abi.BOUNCE_UNIFORM, _abi.DIRECT_RAYS), (_abi.BOUNCE_COSINE, _abi.DIRECT_RAYS), (_abi.BOUNCE_COSINE, _abi.DIRECT_MIS))}
    assert set(new) == want
    assert dbg.jade_debug_shade_mode_passes_host(0, 0, 0, 0, 0, 0, 1, None) == _abi.JADE_ERR_INVALID


def test_the_names_and_the_indices():
    lib = C.CDLL(os.path.join(ROOT, "jaderaytracerendering_amd", "lib", "libjade_hip.so"))
    lib.jade_pass_name.restype = C.c_char_p
    lib.jade_pass_name.argtypes = [C.c_int]
    assert [lib.jade_pass_name(i).decode() for i in range(_abi.PASS_COUNT)] == list(NAMES)
    assert lib.jade_pass_name(-1) is None and lib.jade_pass_name(_abi.PASS_COUNT) is None
    assert NAMES[:3] == ("background", "emission", "specular_sky") and NAMES[3] == "diffuse_emitter_first" and NAMES[-1] == "bssrdf_sky_later"
    assert NAMES[PS.pass_index(1, 1, 0)] == "sss_sky_first" and NAMES[PS.pass_index(2, 0, 1)] == "bssrdf_emitter_later"
