"""Pins the jade branches independently of the oracle's source: single-sample renders (spp = 1, known Wang stream)
against tests/jade_spec.py, a float64 evaluation written from SURVEY.md section 9.  Covers what the closed forms of
test_oracle_units.py do not: the BSSRDF branch (profile, Fi, Fo = R0 - ..., area search returning the last `mid`,
the .A.2/0.9.k/0.5 rate), SSS-diffuse (albedo for direct light, brdf for the indirect rate) and direct refraction
(gen_refract_ray, rate^distance, x5 / x1.25, an open surface => 0).  PathTrace.cu:1029-1178, 931-1028, 1180-1262, 876-894.

The reference itself ships no fixture that could pin these: parity stays "unpinned by the
reference"; what this adds is a second, independently written statement of the same formulas in another precision.
A sample counts as agreeing when every channel is within 1e-4 relative (north_star's tolerance; fp32 + own libm vs
float64 + numpy - measured worst case 5e-6); up to 2 % may disagree (a decision that fp32 and fp64 take differently, such
as a shadow ray grazing an edge - none does at the time of writing).  Samples whose BSSRDF exit point lies in the plane
of the entry point are left out: the reference decides two ray sides there by the sign of rounding noise (jade_spec.bssrdf).

Under a TEXTURED sky (an 8 x 4 map with one bright texel; tests/env_spec.py's float64 lookup) the same comparison runs on the jade
cube and on an open floor, in the reference's mode on both backends and with env_sampling = JADE_ENV_IMPORTANCE - which the oracle
refuses - on the HIP module alone: there jade_spec follows include/jade_rt.h through tests/env_importance_spec.py, sample for sample.

The `patchwork` kind gives the cube's triangles four different materials: what shading reads per TRIANGLE (the module: through its
de-duplicated material table) and what it reads per object must not be confused by either backend.

The scenes, compare() and the one-light cases with their `need` tables (LIGHT_CASES) are in tests/spec_scenes.py: compare() also takes
light_sampling = JADE_LIGHTS_ONE (the HIP module alone; jade_spec's arm of that name), the device comparison is section 7 of
tests/test_gpu_lights.py and the arm's own checks and counts are tests/test_lights_spec_cpu.py."""
import numpy as np
import pytest

import jade_spec
from conftest import B
from jaderaytracerendering_amd import _abi, host as H
from spec_scenes import build, compare

CASES = {
    "jade_cube": dict(size=12, frames=(0, 1, 2), need={"bssrdf": 15, "sss": 30, "mirror": 50, "diffuse": 150}),
    "jade_fold": dict(size=12, frames=(0, 1, 2), need={"bssrdf": 20, "sss": 30, "mirror": 50}),
    "glass_cube": dict(size=12, frames=(0, 1, 2), need={"refract": 40, "refract-open": 2, "mirror": 40}),
    # per-triangle materials (spec_scenes.patchwork).  `need`: half of what jade_spec alone counts per branch on these pixels - 308 diffuse,
    # 50 mirror, 10 refract, 202 sky, 18 sss, 6 bssrdf (7 more leave through their own face and are left out), 1 refract-open
    "patchwork": dict(size=12, frames=(0, 1, 2, 3), need={"bssrdf": 3, "diffuse": 154, "mirror": 25, "refract": 5, "sky": 101, "sss": 9}),
}


@pytest.mark.parametrize("kind", sorted(CASES))
def test_oracle_matches_float64_spec(oracle, kind):
    compare(oracle, kind, **CASES[kind])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", sorted(CASES))
def test_hip_matches_float64_spec(hip, kind):
    compare(hip, kind, **CASES[kind])


# Under the textured sky.  `need`: half of what jade_spec alone counts on these pixels (all of them agree on the oracle in the reference's mode).
SKY_CASES = {
    ("jade_cube", "reference"): dict(size=12, frames=(0, 1, 2), need={"diffuse": 110, "bssrdf": 9, "mirror": 31, "sss": 18, "sky": 76}),
    ("open_floor", "reference"): dict(size=12, frames=(0, 1, 2), need={"diffuse": 119, "sky": 95}),
    ("jade_cube", "importance"): dict(size=12, frames=(0, 1, 2), need={"diffuse": 110, "bssrdf": 7, "mirror": 32, "sss": 21, "sky": 76,
                                                                         "env-importance": 88, "env-noenv": 48}),
    ("open_floor", "importance"): dict(size=12, frames=(0, 1, 2), need={"diffuse": 119, "sky": 95, "env-importance": 79, "env-noenv": 40}),
}
ENV_MODES = {"reference": _abi.ENV_REFERENCE, "importance": _abi.ENV_IMPORTANCE}


@pytest.mark.parametrize("kind", ["jade_cube", "open_floor"])
def test_oracle_matches_float64_spec_under_a_textured_sky(oracle, kind):
    seen, bad, n, skipped = compare(oracle, kind, sky=True, **SKY_CASES[kind, "reference"])
    assert bad == 0, "the map was chosen so that no sample disagrees on the oracle"


@pytest.mark.gpu
@pytest.mark.parametrize("kind,mode", sorted(SKY_CASES))
def test_hip_matches_float64_spec_under_a_textured_sky(hip, kind, mode):
    compare(hip, kind, sky=True, env_sampling=ENV_MODES[mode], **SKY_CASES[kind, mode])


def test_importance_spec_needs_no_gpu_and_the_oracle_refuses_the_mode(oracle):
    """jade_spec's importance arm runs on the CPU (its table comes from the host); the oracle states the reference's estimator only."""
    hs = build("open_floor", sky=True)
    S = jade_spec.Scene(hs, _abi.ENV_IMPORTANCE)
    eye, cam = H.camera_orbit(2.8, 20.0, 10.0)
    tr = []
    for x in range(12):
        assert np.isfinite(jade_spec.sample(S, x, 2, 12, 12, eye, cam, 0, tr)).all()
    assert "env-importance" in tr and "env-noenv" in tr
    with oracle.scene(hs) as so:
        with pytest.raises(B.JadeError) as ei:
            so.render(B.make_params(12, 12, 1, eye, cam, threads=2, env_sampling=_abi.ENV_IMPORTANCE))
    assert ei.value.code == _abi.JADE_ERR_UNSUPPORTED
