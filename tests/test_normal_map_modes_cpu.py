"""Normal maps in the mode rule (shade_mode_for, csrc/jade_runtime.h; include/jade_bvh.h, "The mapped normal, stated"), through
jade_debug_shade_mode_normal_maps_host of libjade_hip_debug.so - host arithmetic, no HIP call, no GPU.  A table in which a triangle is
mapped raises SM_NMAP and, with it, SM_TEX | SM_SMOOTH - a mapped render runs the textured family whatever else the handle carries; it is
built for the reference estimator, for the cosine bounce and under a lens, each with the three environment samplings - nine modes - and
refused by name where textures are: after every other mode's own refusal, whose text stays, in the words of smooth shading or of textures
where the handle carries those and in its own name otherwise.  A table that maps no triangle raises nothing, and the two older entries
answer as they did."""
import ctypes as C
import itertools
import os

import pytest

from conftest import ROOT
from jaderaytracerendering_amd import _abi

ENVIS, LENS, SHUTTER, LIGHTS, COSINE, MIS, ENVMIX, PASSES, BRANCH, SMOOTH, TEX, NMAP = (1 << i for i in range(12))
ENV_BITS = {_abi.ENV_REFERENCE: 0, _abi.ENV_IMPORTANCE: ENVIS, _abi.ENV_MIXTURE: ENVIS | ENVMIX}
# (lens, shutter, lights, bounce, direct, passes, branch) -> bits, for the three accepted rows
ROWS = {
    "maps":        ((0, 0, _abi.LIGHTS_ALL, _abi.BOUNCE_UNIFORM, _abi.DIRECT_RAYS, 0, _abi.BRANCH_RANDOM), NMAP | TEX | SMOOTH),
    "maps+cosine": ((0, 0, _abi.LIGHTS_ALL, _abi.BOUNCE_COSINE, _abi.DIRECT_RAYS, 0, _abi.BRANCH_RANDOM), NMAP | TEX | SMOOTH | COSINE),
    "maps+lens":   ((1, 0, _abi.LIGHTS_ALL, _abi.BOUNCE_UNIFORM, _abi.DIRECT_RAYS, 0, _abi.BRANCH_RANDOM), NMAP | TEX | SMOOTH | LENS),
}
ALL = list(itertools.product((0, 1), (0, 1), (_abi.LIGHTS_ALL, _abi.LIGHTS_ONE), (_abi.BOUNCE_UNIFORM, _abi.BOUNCE_COSINE),
                             (_abi.DIRECT_RAYS, _abi.DIRECT_MIS), (0, 1), (_abi.BRANCH_RANDOM, _abi.BRANCH_STRATIFIED)))
OWN = {"a shutter (jade_scene_set_shutter)", "JADE_LIGHTS_ONE", "JADE_DIRECT_MIS", "passes (jade_scene_set_passes)", "JADE_BRANCH_STRATIFIED"}
HEAD_S = "smooth shading (jade_scene_set_vertex_normals) does not run "
HEAD_T = "textures (jade_scene_set_textures) do not run "
HEAD_N = "normal maps (jade_scene_set_normal_maps) do not run "


@pytest.fixture(scope="module")
def dbg():
    path = os.path.join(ROOT, "jaderaytracerendering_amd", "lib", "libjade_hip_debug.so")
    assert os.path.exists(path), "libjade_hip_debug.so missing: run `make hipvariants` (or __graft_entry__.build())"
    lib = C.CDLL(path)
    for name, n in (("jade_debug_shade_mode_normal_maps_host", 11), ("jade_debug_shade_mode_textures_host", 10), ("jade_debug_shade_mode_smooth_host", 9)):
        getattr(lib, name).restype = C.c_int
        getattr(lib, name).argtypes = [C.c_int32] * n + [C.POINTER(C.c_uint32)]
    lib.jade_last_error.restype = C.c_char_p
    return lib


def _ask(dbg, name, *args):
    mode = C.c_uint32(0xdeadbeef)
    rc = getattr(dbg, name)(*args, C.byref(mode))
    return rc, mode.value, (dbg.jade_last_error() or b"").decode()


def ask(dbg, env, combo, smooth, textures, maps):
    return _ask(dbg, "jade_debug_shade_mode_normal_maps_host", env, *combo, smooth, textures, maps)


def ask_textures(dbg, env, combo, smooth, textures):
    return _ask(dbg, "jade_debug_shade_mode_textures_host", env, *combo, smooth, textures)


def ask_smooth(dbg, env, combo, smooth):
    return _ask(dbg, "jade_debug_shade_mode_smooth_host", env, *combo, smooth)


@pytest.mark.parametrize("env", sorted(ENV_BITS))
@pytest.mark.parametrize("row", sorted(ROWS))
def test_the_nine_modes_are_accepted_with_their_bits_whatever_else_the_handle_carries(dbg, env, row):
    combo, bits = ROWS[row]
    for smooth, textures in itertools.product((0, 1), (0, 1)):
        rc, mode, _ = ask(dbg, env, combo, smooth, textures, 1)
        assert rc == _abi.JADE_OK and mode == bits | ENV_BITS[env], (smooth, textures, mode)


@pytest.mark.parametrize("env", sorted(ENV_BITS))
@pytest.mark.parametrize("smooth,textures", list(itertools.product((0, 1), (0, 1))))
def test_every_other_combination_is_refused_where_textures_are_and_in_the_stated_words(dbg, env, smooth, textures):
    accepted = {c for c, _ in ROWS.values()}
    n_own = n_others = 0
    for combo in ALL:
        rc_t, _, text_t = ask_textures(dbg, env, combo, 0, 1)         # the textures' refusal of the same settings
        rc_0, _, text_0 = ask_smooth(dbg, env, combo, 0)              # ... and what the settings alone are told
        rc, mode, text = ask(dbg, env, combo, smooth, textures, 1)
        if combo in accepted:
            assert rc == _abi.JADE_OK and rc_t == _abi.JADE_OK
            continue
        assert rc == _abi.JADE_ERR_UNSUPPORTED and rc_t == _abi.JADE_ERR_UNSUPPORTED and mode == 0xdeadbeef, (combo, "refused, and the mode left alone")
        if rc_0 != _abi.JADE_OK:                 # refused without any table as well: the same words
            assert text == text_0, (combo, text, text_0)
            n_others += 1
            continue
        n_own += 1
        assert "not built" in text and sum(w in text for w in OWN) == 1, text
        assert text_t.startswith(HEAD_T)
        head = HEAD_S if smooth else HEAD_T if textures else HEAD_N
        assert text == head + text_t[len(HEAD_T):], (text, text_t)
    assert (n_own, n_others) == (13, 112), (n_own, n_others)     # (tests/test_texture_modes_cpu.py counts the same rows)


def test_a_table_that_maps_no_triangle_raises_no_mode_and_the_older_entries_answer_as_before(dbg):
    for env in ENV_BITS:
        for combo in ALL:
            for smooth, textures in itertools.product((0, 1), (0, 1)):
                assert ask(dbg, env, combo, smooth, textures, 0) == ask_textures(dbg, env, combo, smooth, textures)
            for smooth in (0, 1):
                assert ask_textures(dbg, env, combo, smooth, 0) == ask_smooth(dbg, env, combo, smooth)
    # ... and their answers carry no bit of the new mode
    for env in ENV_BITS:
        rc, mode, _ = ask_textures(dbg, env, ROWS["maps"][0], 1, 1)
        assert rc == _abi.JADE_OK and mode == (TEX | SMOOTH | ENV_BITS[env])
        rc, mode, _ = ask_smooth(dbg, env, ROWS["maps"][0], 1)
        assert rc == _abi.JADE_OK and mode == (SMOOTH | ENV_BITS[env])
