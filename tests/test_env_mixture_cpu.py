"""JADE_ENV_MIXTURE without a GPU: the float64 statement tests/env_mixture_spec.py held to what include/jade_rt.h claims of it - the
bounds on m, the mixture's density integrating to 1, an unbiased estimate, the second moment at most twice that of either technique -
on the maps of tests/env_importance_spec.py, with the module's own tables (jade_debug_env_alias_host: host arithmetic, no HIP call);
the conditions the device tests' inputs must meet (ambiguous texels, the `need` tables); and the mode rule over all 96 combinations
(jade_debug_shade_mode_env_host).  tests/test_gpu_env_mixture.py compares the device with the statement."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import env_importance_spec as EI
import env_mixture_cases as MC
import env_mixture_spec as spec
from conftest import ROOT
from jaderaytracerendering_amd import _abi

F32 = np.float32
E = 2.0 ** -24
UNI, COS = spec.UNIFORM, spec.COSINE
ENVIS, LENS, SHUTTER, LIGHTS, COSINE, MIS, ENVMIX = 1, 2, 4, 8, 16, 32, 64
# the nine rows that are built (tests/test_shade_modes_cpu.py spells them out for two environment samplings): (lens, shutter, light
# sampling, bounce sampling, direct sampling) -> the mode's bits
ROWS = {
    (0, 0, _abi.LIGHTS_ALL, _abi.BOUNCE_UNIFORM, _abi.DIRECT_RAYS): 0,
    (1, 0, _abi.LIGHTS_ALL, _abi.BOUNCE_UNIFORM, _abi.DIRECT_RAYS): LENS,
    (0, 1, _abi.LIGHTS_ALL, _abi.BOUNCE_UNIFORM, _abi.DIRECT_RAYS): SHUTTER,
    (1, 1, _abi.LIGHTS_ALL, _abi.BOUNCE_UNIFORM, _abi.DIRECT_RAYS): SHUTTER | LENS,
    (0, 0, _abi.LIGHTS_ONE, _abi.BOUNCE_UNIFORM, _abi.DIRECT_RAYS): LIGHTS,
    (0, 0, _abi.LIGHTS_ALL, _abi.BOUNCE_COSINE, _abi.DIRECT_RAYS): COSINE,
    (0, 0, _abi.LIGHTS_ONE, _abi.BOUNCE_COSINE, _abi.DIRECT_RAYS): COSINE | LIGHTS,
    (0, 0, _abi.LIGHTS_ALL, _abi.BOUNCE_COSINE, _abi.DIRECT_MIS): COSINE | MIS,
    (0, 0, _abi.LIGHTS_ONE, _abi.BOUNCE_COSINE, _abi.DIRECT_MIS): COSINE | MIS | LIGHTS,
}
ENV_BITS = {0: 0, 1: ENVIS, 2: ENVIS | ENVMIX}


@pytest.fixture(scope="module")
def debug_lib():
    path = os.path.join(ROOT, "jaderaytracerendering_amd", "lib", "libjade_hip_debug.so")
    assert os.path.exists(path), "libjade_hip_debug.so missing: run `make hipvariants` (or __graft_entry__.build())"
    lib = C.CDLL(path)
    lib.jade_last_error.restype = C.c_char_p
    return lib


_tables = {}


def table_of(lib, w, h, kind):
    if (w, h, kind) not in _tables:
        _tables[w, h, kind] = EI.table_of(lib, EI.make_map(w, h, kind))
    return _tables[w, h, kind]


def luminance(w, h, kind):
    """L per texel for the integrals below: the luminance the table was made from (0 where a channel is not finite) - constant per texel."""
    env = EI.make_map(w, h, kind).astype(np.float64)
    with np.errstate(all="ignore"):
        c = np.where(env < 0, 0.0, env)
        lum = 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]
    return np.where(np.isfinite(lum), lum, 0.0).ravel()


def quadrature(w, h):
    """At least 512 x 256 points over the map, a whole number per texel."""
    return spec.Quadrature(w, h, -(-512 // w), -(-256 // h))


# the surfaces of the integral tests: looking up, sideways, down, and a tilted normal of length 2.5 seen from behind
SURFACES = [((0, 1, 0), 1.0), ((1, 0, 0), 1.0), ((0, -1, 0), 1.0), ((0.75, 1.5, -1.85), -1.0)]
MAP_IDS = [f"{w}x{h}-{k}" for w, h, k in MC.MAPS]


@pytest.mark.parametrize("w,h,kind", MC.MAPS, ids=MAP_IDS)
def test_the_weight_stays_within_its_bounds(debug_lib, w, h, kind):
    """m >= 0; m <= 2 in the uniform form and m c <= 1 in the cosine form, up to 4 roundings - on the device tests' own rows, which hold
    every normal of the list (zero, NaN and inf among them: those take the uniform form) with both sides."""
    t = table_of(debug_lib, w, h, kind)
    for tech in (UNI, COS):
        r = MC.rows(t, w, h, tech)
        d = MC.spec_draw(t, w, h, r, tech)
        m, cf = d["m"], d["cosine_form"]
        assert np.isfinite(m).all() and (m >= 0).all()
        assert (m[~cf] <= 2 * (1 + 4 * E)).all(), float(m[~cf].max())
        assert (tech == COS) == bool(cf.any())
        if cf.any():
            assert ((m * d["c"])[cf] <= 1 + 4 * E).all(), float((m * d["c"])[cf].max())
        pole = d["s"] == 0
        assert (m[pole] == 0).all()
        assert not (d["wrong"] & d["hemi"]).any() and d["wrong"].sum() > 100 and (d["own"] & ~d["hemi"]).sum() > 100


@pytest.mark.parametrize("w,h,kind", MC.MAPS, ids=MAP_IDS)
def test_the_mixtures_density_integrates_to_one_and_the_second_moment_theorem_holds(debug_lib, w, h, kind):
    """p_sky / 2 + p_hemi / 2 integrates to 1 over the sphere (the indicator of a hemisphere costs the midpoint rule a cell's width along
    its edge: 1 % allowed), and E[X^2] of the mixture is at most twice that of either technique alone - both by quadrature."""
    t = table_of(debug_lib, w, h, kind)
    Q = quadrature(w, h)
    lum = luminance(w, h, kind)[Q.texel]
    for n, side in SURFACES:
        for tech in (UNI, COS):
            ps, ph = spec.densities(Q, t, F32(n), side, tech)
            assert abs(Q.integral(ps) - 1) < 1e-5 and abs(Q.integral(ph) - 1) < 1e-2, (Q.integral(ps), Q.integral(ph))
            assert abs(Q.integral(0.5 * ps + 0.5 * ph) - 1) < 1e-2
            I, sky2, hemi2, mix2 = spec.moments(Q, t, lum, F32(n), side, tech)
            assert mix2 <= 2 * min(sky2, hemi2) * (1 + 1e-12), (n, side, tech, sky2, hemi2, mix2)
            assert mix2 >= I * I * (1 - 1e-9)


@pytest.mark.parametrize("w,h,kind", MC.MAPS, ids=MAP_IDS)
def test_the_estimate_is_unbiased(debug_lib, w, h, kind):
    """The mean of 200 000 draws of L |n.w| 2 pi m (0 for a sky draw on the wrong side) equals the quadrature of the integral of
    L |n.w| over the hemisphere within 5 standard errors, the standard error from the quadrature's second moment."""
    t = table_of(debug_lib, w, h, kind)
    Q = quadrature(w, h)
    lum_t = luminance(w, h, kind)
    k = 200000
    for si, (n, side) in enumerate(SURFACES):
        for tech in (UNI, COS):
            rng = np.random.default_rng(1000 * si + tech)
            u = (rng.integers(0, 2 ** 32, size=(k, 5), dtype=np.uint64).astype(F32) * F32(2.0 ** -32)).astype(F32)
            d = spec.draw(t, w, h, np.tile(F32(n), (k, 1)), np.full(k, side, F32), tech, *u.T)
            n64 = np.asarray(F32(n), np.float64)
            x = np.where(d["wrong"], 0.0, lum_t[d["texel"]] * np.abs(d["d"] @ n64) * 2 * spec.PI * d["m"])
            I, _, _, mix2 = spec.moments(Q, t, lum_t[Q.texel], F32(n), side, tech)
            se = np.sqrt(max(mix2 - I * I, 0.0) / k)
            assert abs(x.mean() - I) <= 5 * se, (n, side, tech, float(x.mean()), I, se)


@pytest.mark.parametrize("w,h,kind", MC.MAPS, ids=MAP_IDS)
def test_few_hemisphere_rows_have_an_ambiguous_texel(debug_lib, w, h, kind):
    """A condition on the device test's inputs: at most 1 % of a map's hemisphere rows lie within delta of a texel's border (the rows
    placed there on purpose included)."""
    t = table_of(debug_lib, w, h, kind)
    for tech in (UNI, COS):
        r = MC.rows(t, w, h, tech)
        assert len(r) >= 20000
        d = MC.spec_draw(t, w, h, r, tech)
        hemi = d["hemi"]
        amb = spec.set_size(d["u"], d["v"], w, h, d["du"], d["dv"])[hemi] > 1
        assert hemi.sum() > 9000 and amb.mean() <= 0.01, (tech, int(amb.sum()), int(hemi.sum()))
        if w * h > 1:
            assert amb.sum() >= 8, "the border rows are among them"
        # rows whose flip (hemisphere) or wrong-side test (sky) is decided by a product within rounding of 0: few, and the infinite
        # normal's rows are not among them unless the component its infinity multiplies lies within the direction's bound of 0
        inf_n = np.isinf(r[:, 5:8]).any(1)
        assert d["unsure"].mean() <= 0.03 and (d["unsure"] & hemi).sum() <= 0.01 * hemi.sum()
        assert inf_n.sum() > 900 and (d["unsure"] & inf_n).sum() <= 0.1 * inf_n.sum()


def test_texel_of_a_direction():
    """Centres and corners of an 8 x 4 map, the poles, the seam, and what is not a direction."""
    w, h = 8, 4
    uu, vv = np.meshgrid((np.arange(w) + 0.5) / w, (np.arange(h) + 0.5) / h)
    d = EI.direction_of(uu.ravel(), vv.ravel())[0]
    assert np.array_equal(spec.texel_of(d, w, h)[0], np.arange(w * h))
    assert spec.texel_of([[0, 1, 0]], w, h)[0][0] == w // 2 and spec.texel_of([[0, -1, 0]], w, h)[0][0] == (h - 1) * w + w // 2
    t, u, v = spec.texel_of([[-1, 0, 1e-9], [-1, 0, -1e-9], [-1, 0, 0.0]], w, h)
    assert t[0] % w == w - 1 and t[1] % w == 0
    du, dv = spec.deltas([[-1, 0, 1e-9]], w, h)
    assert spec.accepts([t[1]], u[:1], v[:1], w, h, du, dv)[0] and spec.set_size(u[:1], v[:1], w, h, du, dv)[0] == 4   # (the seam, on a row border)
    assert (spec.texel_of([[0, 0, 0], [np.nan, 1, 0]], w, h)[0] == 0).all()


ALL96 = list(itertools.product((0, 1, 2), (0, 1), (0, 1), (_abi.LIGHTS_ALL, _abi.LIGHTS_ONE), (_abi.BOUNCE_UNIFORM, _abi.BOUNCE_COSINE),
                               (_abi.DIRECT_RAYS, _abi.DIRECT_MIS)))


def test_the_mode_rule_over_all_96_combinations(debug_lib):
    """27 accepted with their bits; the 0 / 1 columns are jade_debug_shade_mode_host's answers; the mixture's refusals are importance's,
    word for word; every other value of env_sampling is JADE_ERR_INVALID."""
    lib = debug_lib
    lib.jade_debug_shade_mode_host.restype = C.c_int
    lib.jade_debug_shade_mode_host.argtypes = [C.c_int32] * 6 + [C.POINTER(C.c_uint32)]
    assert len(ALL96) == 96
    accepted = {}
    text = {}
    for combo in ALL96:
        rc, mode = spec.shade_mode_env(lib, combo)
        text[combo] = (rc, (lib.jade_last_error() or b"").decode() if rc else "")
        if rc == 0:
            accepted[combo] = mode
        else:
            assert rc == _abi.JADE_ERR_UNSUPPORTED
        if combo[0] < 2:
            old = C.c_uint32(0xdeadbeef)
            rc_old = lib.jade_debug_shade_mode_host(*combo, C.byref(old))
            assert rc_old == rc and (rc != 0 or old.value == mode)
            assert rc == 0 or (lib.jade_last_error() or b"").decode() == text[combo][1]
    assert len(accepted) == 27 and len(set(accepted.values())) == 27
    assert set(accepted) == {(env,) + row for env in (0, 1, 2) for row in ROWS}
    for combo, mode in accepted.items():
        assert mode == ROWS[combo[1:]] | ENV_BITS[combo[0]], (combo, mode)
    for combo in ALL96:
        if combo[0] == 2:
            assert text[combo] == text[(1,) + combo[1:]], combo
    for bad in (3, -1, 255):
        rc, _ = spec.shade_mode_env(lib, (bad, 0, 0, 0, 0, 0))
        assert rc == _abi.JADE_ERR_INVALID
    lib.jade_debug_shade_mode_env_host.argtypes = [C.c_int32] * 6 + [C.c_void_p]
    assert lib.jade_debug_shade_mode_env_host(2, 0, 0, 0, 0, 0, None) == _abi.JADE_ERR_INVALID


def test_the_map_size_predicate_is_importances(debug_lib):
    fits = debug_lib.jade_debug_env_importance_fits
    fits.restype, fits.argtypes = C.c_int, [C.c_int32, C.c_int32]
    assert fits(4096, 4096) == 1 and fits(8192, 4096) == 0 and fits(0, 4) == 0
    assert _abi.ENV_MIXTURE == 2 and (_abi.ENV_REFERENCE, _abi.ENV_IMPORTANCE) == (0, 1)
    text = open(os.path.join(ROOT, "include", "jade_rt.h")).read()
    assert "#define JADE_ENV_MIXTURE 2" in text


def test_the_row_check_refuses_what_would_index_past_the_table(debug_lib):
    """jade_debug_env_mix_rows: a uniform outside [0, 1] (a NaN is), an unknown technique, a wrong width - refused on the host."""
    fn = debug_lib.jade_debug_env_mix_rows
    fn.restype, fn.argtypes = C.c_int, [C.c_int32, C.c_int32, C.c_void_p]
    good = spec.rows_of(np.full((3, 5), 0.25, F32), [0, 1, 0], 1.0, COS)
    assert fn(3, 10, good.ctypes.data) == 0
    for col, val in ((1, 1.5), (0, -0.1), (4, np.nan), (9, 2.0), (9, 0.5)):
        bad = good.copy()
        bad[1, col] = val
        assert fn(3, 10, bad.ctypes.data) == _abi.JADE_ERR_INVALID, (col, val)
    anything = good.copy()
    anything[:, 5:9] = np.nan
    assert fn(3, 10, anything.ctypes.data) == 0, "the normal and the side form no index"
    assert fn(3, 9, good.ctypes.data) == _abi.JADE_ERR_INVALID and fn(0, 10, good.ctypes.data) == _abi.JADE_ERR_INVALID
    assert fn(3, 10, None) == _abi.JADE_ERR_INVALID


@pytest.mark.parametrize("name", sorted(MC.ARMS))
def test_the_need_tables_are_half_of_what_the_arm_alone_counts(name):
    """... and the arm alone leaves out at most 5 % of the samples (coplanar BSSRDF exits, hemisphere draws with an ambiguous texel)."""
    seen, bad, n, skipped = MC.compare(None, name, count_only=True)
    assert bad == 0 and skipped <= MC.MAX_LEFT_OUT * (n + skipped)
    need = MC.ARMS[name]["need"]
    assert set(MC.MIX_TAGS) <= set(need)
    assert need == {tag: count // 2 for tag, count in seen.items() if count // 2 > 0}, dict(sorted(seen.items()))
