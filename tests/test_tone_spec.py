"""The tone curve and byte pack against the float64 statement of tests/tone_spec.py, without a GPU: the oracle's
(jade_oracle_tone_pack: the statements jade_render_resolve_ex runs) and the HIP module's own tone_pack_bgr8 compiled for the host
(jade_debug_tone_pack_host: what jade_render_multi packs its gathered frame with), which must also agree with each other on every
input.  tests/test_gpu_tone.py asks the same of tone_pack_bgr8 on the device."""
import numpy as np
import pytest

import tone_spec
from tone_spec import SPECIAL_ROWS, host_tone_pack, oracle_tone_pack, special_bytes

@pytest.mark.parametrize("tonemap,limit", tone_spec.CASES)
def test_oracle_tone_bytes_equal_the_float64_statement(oracle, tonemap, limit):
    rgb, n_gen = tone_spec.inputs(tonemap, limit)
    assert 250000 <= len(rgb) <= 350000
    got = oracle_tone_pack(oracle, rgb, tonemap, limit)
    tone_spec.check_bytes(got, rgb, tonemap, limit, n_gen)


@pytest.mark.parametrize("tonemap,limit", tone_spec.CASES)
def test_host_copy_of_the_hip_tone_curve_equals_the_oracle_and_the_float64_statement(oracle, tonemap, limit):
    """jade_render_multi tone-maps on the host; its bytes must be k_resolve's and the oracle's - the special and huge rows included."""
    rgb, n_gen = tone_spec.inputs(tonemap, limit)
    got = host_tone_pack(rgb, tonemap, limit)
    want = oracle_tone_pack(oracle, rgb, tonemap, limit)
    bad = np.flatnonzero((got != want).any(1))
    assert len(bad) == 0, [(rgb[i].tolist(), got[i].tolist(), want[i].tolist()) for i in bad[:5]]
    tone_spec.check_bytes(got, rgb, tonemap, limit, n_gen)


def test_oracle_tone_pack_special_values(oracle):
    assert oracle_tone_pack(oracle, SPECIAL_ROWS, tone_spec.ACES, 0.0).tolist() == special_bytes()
    with pytest.raises(Exception):
        oracle_tone_pack(oracle, SPECIAL_ROWS, 7, 1.5)


def test_host_copy_tone_pack_special_values():
    assert host_tone_pack(SPECIAL_ROWS, tone_spec.ACES, 0.0).tolist() == special_bytes()
    with pytest.raises(Exception):
        host_tone_pack(SPECIAL_ROWS, 7, 1.5)
