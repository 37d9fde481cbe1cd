"""The seams of the render modes on the device: every check of tests/mode_seams.py for every case of its table - the lens, the shutter,
both, one-light sampling, cosine bounces, MIS.  What is particular to a mode is in its own file (test_gpu_lens.py, test_gpu_shutter.py,
test_gpu_lights.py, test_gpu_bounce.py, test_gpu_mis.py)."""
import pytest

import mode_seams as MS

pytestmark = pytest.mark.gpu

ALL_CASES = [c.name for c in MS.CASES]


@pytest.fixture
def ref(hip, case):
    """The case's reference render, made once per run of this module."""
    return MS.reference(hip, MS.BY_NAME[case])


@pytest.mark.parametrize("case", ALL_CASES)
def test_the_same_bits_and_counters_twice(hip, ref, case):
    MS.check_twice(hip, MS.BY_NAME[case], ref)


@pytest.mark.parametrize("case", ALL_CASES)
def test_the_same_bits_under_the_three_walks(hip, ref, case):
    MS.check_walks(hip, MS.BY_NAME[case], ref)


@pytest.mark.parametrize("case", ALL_CASES)
def test_steps_and_a_flush_equal_one_call(hip, ref, case):
    MS.check_steps(hip, MS.BY_NAME[case], ref)


@pytest.mark.parametrize("case", ALL_CASES)
def test_tile_shares_assemble_to_the_frame(hip, ref, case):
    MS.check_shares(hip, MS.BY_NAME[case], ref)


@pytest.mark.parametrize("case,env", [pytest.param(c.name, env, id=f"{c.name}-{MS.schedule_id(env)}") for c in MS.CASES for env in MS.schedules(c)])
def test_schedules_are_one_result(hip, ref, monkeypatch, case, env):
    MS.check_schedule(hip, MS.BY_NAME[case], ref, env, monkeypatch.setenv)


@pytest.mark.parametrize("case", MS.SAMPLING)
def test_an_unknown_value_is_invalid_and_leaves_the_setting(hip, case):
    MS.check_unknown_value(hip, MS.BY_NAME[case])


@pytest.mark.parametrize("case", ALL_CASES)
def test_the_oracle_has_no_such_entry_point(oracle, case):
    MS.check_oracle_refuses(oracle, MS.BY_NAME[case])


@pytest.mark.parametrize("case", ALL_CASES)
def test_render_multi_takes_equal_settings_and_refuses_unequal_ones(hip, ref, case):
    MS.check_render_multi(hip, MS.BY_NAME[case], ref)


@pytest.mark.parametrize("case", MS.SAMPLING)
def test_a_refusal_leaves_the_handle_usable(hip, ref, case):
    MS.check_refusal_leaves_the_handle_usable(hip, MS.BY_NAME[case], ref)


@pytest.mark.parametrize("case", MS.SAMPLING)
def test_the_command_line(case, tmp_path):
    MS.check_command_line(MS.BY_NAME[case], tmp_path)
