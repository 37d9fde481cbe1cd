"""Textures in the mode rule (shade_mode_for, csrc/jade_runtime.h; include/jade_bvh.h, "The surface colour, stated"), through
jade_debug_shade_mode_textures_host of libjade_hip_debug.so - host arithmetic, no HIP call, no GPU.  A table in which a triangle names an
image raises SM_TEX and, with it, SM_SMOOTH - a textured render runs the smooth family whether the handle carries vertex normals or not;
it is built for the reference estimator, for the cosine bounce and under a lens, each with the three environment samplings, and refused
by name - after every other mode's own refusal, whose text stays, and in smooth shading's words - with a shutter, JADE_LIGHTS_ONE,
JADE_DIRECT_MIS, passes and JADE_BRANCH_STRATIFIED.  A table that names no image raises nothing."""
import ctypes as C
import itertools
import os

import pytest

from conftest import ROOT
from jaderaytracerendering_amd import _abi

ENVIS, LENS, SHUTTER, LIGHTS, COSINE, MIS, ENVMIX, PASSES, BRANCH, SMOOTH, TEX = (1 << i for i in range(11))
ENV_BITS = {_abi.ENV_REFERENCE: 0, _abi.ENV_IMPORTANCE: ENVIS, _abi.ENV_MIXTURE: ENVIS | ENVMIX}
# (lens, shutter, lights, bounce, direct, passes, branch) -> bits, for the three accepted rows
ROWS = {
    "textures":        ((0, 0, _abi.LIGHTS_ALL, _abi.BOUNCE_UNIFORM, _abi.DIRECT_RAYS, 0, _abi.BRANCH_RANDOM), TEX | SMOOTH),
    "textures+cosine": ((0, 0, _abi.LIGHTS_ALL, _abi.BOUNCE_COSINE, _abi.DIRECT_RAYS, 0, _abi.BRANCH_RANDOM), TEX | SMOOTH | COSINE),
    "textures+lens":   ((1, 0, _abi.LIGHTS_ALL, _abi.BOUNCE_UNIFORM, _abi.DIRECT_RAYS, 0, _abi.BRANCH_RANDOM), TEX | SMOOTH | LENS),
}
ALL = list(itertools.product((0, 1), (0, 1), (_abi.LIGHTS_ALL, _abi.LIGHTS_ONE), (_abi.BOUNCE_UNIFORM, _abi.BOUNCE_COSINE),
                             (_abi.DIRECT_RAYS, _abi.DIRECT_MIS), (0, 1), (_abi.BRANCH_RANDOM, _abi.BRANCH_STRATIFIED)))
OWN = {"a shutter (jade_scene_set_shutter)", "JADE_LIGHTS_ONE", "JADE_DIRECT_MIS", "passes (jade_scene_set_passes)", "JADE_BRANCH_STRATIFIED"}


@pytest.fixture(scope="module")
def dbg():
    path = os.path.join(ROOT, "jaderaytracerendering_amd", "lib", "libjade_hip_debug.so")
    assert os.path.exists(path), "libjade_hip_debug.so missing: run `make hipvariants` (or __graft_entry__.build())"
    lib = C.CDLL(path)
    for name, n in (("jade_debug_shade_mode_textures_host", 10), ("jade_debug_shade_mode_smooth_host", 9)):
        getattr(lib, name).restype = C.c_int
        getattr(lib, name).argtypes = [C.c_int32] * n + [C.POINTER(C.c_uint32)]
    lib.jade_last_error.restype = C.c_char_p
    return lib


def ask(dbg, env, combo, smooth, textures):
    mode = C.c_uint32(0xdeadbeef)
    rc = dbg.jade_debug_shade_mode_textures_host(env, *combo, smooth, textures, C.byref(mode))
    return rc, mode.value, (dbg.jade_last_error() or b"").decode()


def ask_before(dbg, env, combo, smooth):
    """The rule as it was asked before textures: jade_debug_shade_mode_smooth_host."""
    mode = C.c_uint32(0xdeadbeef)
    rc = dbg.jade_debug_shade_mode_smooth_host(env, *combo, smooth, C.byref(mode))
    return rc, mode.value, (dbg.jade_last_error() or b"").decode()


@pytest.mark.parametrize("env", sorted(ENV_BITS))
@pytest.mark.parametrize("row", sorted(ROWS))
@pytest.mark.parametrize("smooth", (0, 1))
def test_the_three_rows_are_accepted_with_vertex_normals_and_without(dbg, env, row, smooth):
    combo, bits = ROWS[row]
    rc, mode, _ = ask(dbg, env, combo, smooth, 1)
    assert rc == _abi.JADE_OK and mode == bits | ENV_BITS[env]


@pytest.mark.parametrize("env", sorted(ENV_BITS))
@pytest.mark.parametrize("smooth", (0, 1))
def test_every_other_combination_is_refused_where_smooth_shading_is_and_in_its_words(dbg, env, smooth):
    accepted = {c for c, _ in ROWS.values()}
    n_own = n_others = 0
    for combo in ALL:
        rc_s, _, text_s = ask_before(dbg, env, combo, 1)            # the smooth table's refusal of the same settings
        rc_0, _, text_0 = ask_before(dbg, env, combo, 0)            # ... and what the settings alone are told
        rc, mode, text = ask(dbg, env, combo, smooth, 1)
        if combo in accepted:
            assert rc == _abi.JADE_OK and rc_s == _abi.JADE_OK
            continue
        assert rc == _abi.JADE_ERR_UNSUPPORTED and rc_s == _abi.JADE_ERR_UNSUPPORTED and mode == 0xdeadbeef, (combo, "refused, and the mode left alone")
        if rc_0 != _abi.JADE_OK:                 # refused without any table as well: the same words
            assert text == text_0, (combo, text, text_0)
            n_others += 1
            continue
        n_own += 1
        assert "not built" in text and sum(w in text for w in OWN) == 1, text
        if smooth:                               # both tables: smooth shading's refusal as it always read
            assert text == text_s
        else:                                    # the same words with the textures for a subject
            head_s, head_t = "smooth shading (jade_scene_set_vertex_normals) does not run ", "textures (jade_scene_set_textures) do not run "
            assert text_s.startswith(head_s) and text == head_t + text_s[len(head_s):], (text, text_s)
    assert (n_own, n_others) == (13, 112), (n_own, n_others)     # (tests/test_smooth_modes_cpu.py counts the same rows)


def test_a_table_that_names_no_image_raises_no_mode(dbg):
    for env in ENV_BITS:
        for combo in ALL:
            for smooth in (0, 1):
                assert ask(dbg, env, combo, smooth, 0) == ask_before(dbg, env, combo, smooth)
