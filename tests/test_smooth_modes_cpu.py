"""Smooth shading in the mode rule (shade_mode_for, csrc/jade_runtime.h; include/jade_bvh.h, "The shading normal, stated"), through
jade_debug_shade_mode_smooth_host of libjade_hip_debug.so - host arithmetic, no HIP call, no GPU.  A table that is not flat everywhere
raises SM_SMOOTH; it is built for the reference estimator, for the cosine bounce and under a lens, each with the three environment
samplings, and refused by name - after every other mode's own refusal, whose text stays - with a shutter, JADE_LIGHTS_ONE, JADE_DIRECT_MIS,
passes, JADE_BRANCH_STRATIFIED, and the cosine bounce under a lens (which the cosine bounce's own check refuses first)."""
import ctypes as C
import itertools
import os

import pytest

from conftest import ROOT
from jaderaytracerendering_amd import _abi

ENVIS, LENS, SHUTTER, LIGHTS, COSINE, MIS, ENVMIX, PASSES, BRANCH, SMOOTH = (1 << i for i in range(10))
ENV_BITS = {_abi.ENV_REFERENCE: 0, _abi.ENV_IMPORTANCE: ENVIS, _abi.ENV_MIXTURE: ENVIS | ENVMIX}
# (lens, shutter, lights, bounce, direct, passes, branch) -> bits, for the three accepted rows
ROWS = {
    "smooth":        ((0, 0, _abi.LIGHTS_ALL, _abi.BOUNCE_UNIFORM, _abi.DIRECT_RAYS, 0, _abi.BRANCH_RANDOM), SMOOTH),
    "smooth+cosine": ((0, 0, _abi.LIGHTS_ALL, _abi.BOUNCE_COSINE, _abi.DIRECT_RAYS, 0, _abi.BRANCH_RANDOM), SMOOTH | COSINE),
    "smooth+lens":   ((1, 0, _abi.LIGHTS_ALL, _abi.BOUNCE_UNIFORM, _abi.DIRECT_RAYS, 0, _abi.BRANCH_RANDOM), SMOOTH | LENS),
}
ALL = list(itertools.product((0, 1), (0, 1), (_abi.LIGHTS_ALL, _abi.LIGHTS_ONE), (_abi.BOUNCE_UNIFORM, _abi.BOUNCE_COSINE),
                             (_abi.DIRECT_RAYS, _abi.DIRECT_MIS), (0, 1), (_abi.BRANCH_RANDOM, _abi.BRANCH_STRATIFIED)))


@pytest.fixture(scope="module")
def dbg():
    path = os.path.join(ROOT, "jaderaytracerendering_amd", "lib", "libjade_hip_debug.so")
    assert os.path.exists(path), "libjade_hip_debug.so missing: run `make hipvariants` (or __graft_entry__.build())"
    lib = C.CDLL(path)
    for name, n in (("jade_debug_shade_mode_smooth_host", 9), ("jade_debug_shade_mode_branch_host", 8)):
        getattr(lib, name).restype = C.c_int
        getattr(lib, name).argtypes = [C.c_int32] * n + [C.POINTER(C.c_uint32)]
    lib.jade_last_error.restype = C.c_char_p
    return lib


def ask(dbg, env, combo, smooth):
    mode = C.c_uint32(0xdeadbeef)
    rc = dbg.jade_debug_shade_mode_smooth_host(env, *combo, smooth, C.byref(mode))
    return rc, mode.value, (dbg.jade_last_error() or b"").decode()


def ask_flat(dbg, env, combo):
    mode = C.c_uint32(0xdeadbeef)
    rc = dbg.jade_debug_shade_mode_branch_host(env, *combo, C.byref(mode))
    return rc, mode.value, (dbg.jade_last_error() or b"").decode()


@pytest.mark.parametrize("env", sorted(ENV_BITS))
@pytest.mark.parametrize("row", sorted(ROWS))
def test_the_three_rows_are_accepted_under_each_environment_sampling(dbg, env, row):
    combo, bits = ROWS[row]
    rc, mode, _ = ask(dbg, env, combo, 1)
    assert rc == _abi.JADE_OK and mode == bits | ENV_BITS[env]


def own_refusal(lens, shutter, lights, bounce, direct, passes, branch):
    """The words of smooth shading's own refusal, in the order the rule asks; None: one of the three rows."""
    if shutter:
        return "a shutter (jade_scene_set_shutter)"
    if lights == _abi.LIGHTS_ONE:
        return "JADE_LIGHTS_ONE"
    if direct == _abi.DIRECT_MIS:
        return "JADE_DIRECT_MIS"
    if passes:
        return "passes (jade_scene_set_passes)"
    if branch == _abi.BRANCH_STRATIFIED:
        return "JADE_BRANCH_STRATIFIED"
    if lens and bounce == _abi.BOUNCE_COSINE:
        return "pinhole"
    return None


@pytest.mark.parametrize("env", sorted(ENV_BITS))
def test_every_other_combination_is_refused_after_everybody_elses_refusal(dbg, env):
    accepted = {c for c, _ in ROWS.values()}
    n_own = n_others = 0
    for combo in ALL:
        rc_flat, mode_flat, text_flat = ask_flat(dbg, env, combo)
        rc, mode, text = ask(dbg, env, combo, 1)
        if combo in accepted:
            assert rc == _abi.JADE_OK
            continue
        assert rc == _abi.JADE_ERR_UNSUPPORTED and mode == 0xdeadbeef, (combo, "refused, and the mode left alone")
        if rc_flat != _abi.JADE_OK:             # refused without a table as well: the same words
            assert text == text_flat, (combo, text, text_flat)
            n_others += 1
        else:
            want = own_refusal(*combo)
            assert want is not None and text.startswith("smooth shading (jade_scene_set_vertex_normals)") and want in text, (combo, text)
            assert "not built" in text
            n_own += 1
    # JADE_SHADE_MODES_BUILT has 16 rows per environment sampling without SM_SMOOTH (twelve, and four under SM_BRANCH); three of them are the
    # accepted rows above, so 13 combinations get smooth shading's own refusal and the other 128 - 16 = 112 keep the text they had
    assert (n_own, n_others) == (13, 112), (n_own, n_others)


def test_each_refusal_text_is_reached(dbg):
    base = list(ROWS["smooth"][0])
    cases = {"a shutter (jade_scene_set_shutter)": (1, 1), "JADE_LIGHTS_ONE": (2, _abi.LIGHTS_ONE), "passes (jade_scene_set_passes)": (5, 1),
             "JADE_BRANCH_STRATIFIED": (6, _abi.BRANCH_STRATIFIED)}
    for want, (i, v) in cases.items():
        c = list(base)
        c[i] = v
        rc, _, text = ask(dbg, _abi.ENV_REFERENCE, c, 1)
        assert rc == _abi.JADE_ERR_UNSUPPORTED and want in text and text.startswith("smooth shading"), text
    mis = list(ROWS["smooth+cosine"][0])
    mis[4] = _abi.DIRECT_MIS
    rc, _, text = ask(dbg, _abi.ENV_REFERENCE, mis, 1)
    assert rc == _abi.JADE_ERR_UNSUPPORTED and "JADE_DIRECT_MIS" in text and text.startswith("smooth shading"), text
    # the cosine bounce under a lens is the cosine bounce's own refusal, smooth or not
    both = list(ROWS["smooth+lens"][0])
    both[3] = _abi.BOUNCE_COSINE
    rc, _, text = ask(dbg, _abi.ENV_REFERENCE, both, 1)
    assert rc == _abi.JADE_ERR_UNSUPPORTED and text.startswith("bounce sampling: JADE_BOUNCE_COSINE") and "lens" in text


def test_without_a_table_nothing_changes(dbg):
    for env in ENV_BITS:
        for combo in ALL:
            assert ask(dbg, env, combo, 0)[:2] == ask_flat(dbg, env, combo)[:2]
