"""Which render modes are built, and what jade_render_begin says about the others: the rule (shade_mode_for, csrc/jade_runtime.h) over all
64 combinations of its six settings, through jade_debug_shade_mode_host of libjade_hip_debug.so - host arithmetic, no HIP call, no GPU.

The rule as include/jade_bvh.h states it, setting by setting:
  * "The lights, stated": jade_render_begin refuses JADE_LIGHTS_ONE with JADE_ERR_UNSUPPORTED together with a lens or a shutter;
  * "The bounce, stated": it refuses JADE_BOUNCE_COSINE with JADE_ERR_UNSUPPORTED together with a lens or a shutter;
  * "The direct light, stated": it refuses JADE_DIRECT_MIS without JADE_BOUNCE_COSINE with JADE_ERR_UNSUPPORTED; a lens or a shutter is
    refused by JADE_BOUNCE_COSINE's own check;
  * a lens, a shutter, both, and either environment sampling run with everything that is not refused above.
The first of these that applies, in this order, is the refusal a caller reads (tests/test_gpu_lights.py, test_gpu_bounce.py and
test_gpu_mis.py read the mode's name and "lens" / "shutter" out of its text).  What is left are 18 modes, spelled out below with the
bits of csrc/jade_runtime.h's ShadeMode."""
import ctypes as C
import itertools
import os

import pytest

from conftest import ROOT
from jaderaytracerendering_amd import _abi

ENVIS, LENS, SHUTTER, LIGHTS, COSINE, MIS = 1, 2, 4, 8, 16, 32

# {reference, importance} x these nine: (lens, shutter, light sampling, bounce sampling, direct sampling) -> the mode's bits
BUILT = {
    "pinhole":          ((0, 0, _abi.LIGHTS_ALL, _abi.BOUNCE_UNIFORM, _abi.DIRECT_RAYS), 0),
    "lens":             ((1, 0, _abi.LIGHTS_ALL, _abi.BOUNCE_UNIFORM, _abi.DIRECT_RAYS), LENS),
    "shutter":          ((0, 1, _abi.LIGHTS_ALL, _abi.BOUNCE_UNIFORM, _abi.DIRECT_RAYS), SHUTTER),
    "shutter+lens":     ((1, 1, _abi.LIGHTS_ALL, _abi.BOUNCE_UNIFORM, _abi.DIRECT_RAYS), SHUTTER | LENS),
    "one-light":        ((0, 0, _abi.LIGHTS_ONE, _abi.BOUNCE_UNIFORM, _abi.DIRECT_RAYS), LIGHTS),
    "cosine":           ((0, 0, _abi.LIGHTS_ALL, _abi.BOUNCE_COSINE, _abi.DIRECT_RAYS), COSINE),
    "cosine+one-light": ((0, 0, _abi.LIGHTS_ONE, _abi.BOUNCE_COSINE, _abi.DIRECT_RAYS), COSINE | LIGHTS),
    "MIS":              ((0, 0, _abi.LIGHTS_ALL, _abi.BOUNCE_COSINE, _abi.DIRECT_MIS), COSINE | MIS),
    "MIS+one-light":    ((0, 0, _abi.LIGHTS_ONE, _abi.BOUNCE_COSINE, _abi.DIRECT_MIS), COSINE | MIS | LIGHTS),
}
ACCEPTED = {(env,) + settings: bits | (ENVIS if env else 0) for env in (0, 1) for settings, bits in BUILT.values()}
ALL = list(itertools.product((0, 1), (0, 1), (0, 1), (_abi.LIGHTS_ALL, _abi.LIGHTS_ONE), (_abi.BOUNCE_UNIFORM, _abi.BOUNCE_COSINE),
                             (_abi.DIRECT_RAYS, _abi.DIRECT_MIS)))


def refusal(env, lens, shutter, lights, bounce, direct):
    """The words a caller must find in the refusal's text, by the header's rule; None: accepted."""
    camera = "lens" if lens else "shutter" if shutter else None
    if lights == _abi.LIGHTS_ONE and camera:
        return ("JADE_LIGHTS_ONE", camera)
    if bounce == _abi.BOUNCE_COSINE and camera:
        return ("JADE_BOUNCE_COSINE", camera)
    if direct == _abi.DIRECT_MIS and bounce != _abi.BOUNCE_COSINE:
        return ("JADE_DIRECT_MIS", "JADE_BOUNCE_COSINE")
    return None


@pytest.fixture(scope="module")
def dbg():
    path = os.path.join(ROOT, "jaderaytracerendering_amd", "lib", "libjade_hip_debug.so")
    assert os.path.exists(path), "libjade_hip_debug.so missing: run `make hipvariants` (or __graft_entry__.build())"
    lib = C.CDLL(path)
    lib.jade_debug_shade_mode_host.restype = C.c_int
    lib.jade_debug_shade_mode_host.argtypes = [C.c_int32] * 6 + [C.POINTER(C.c_uint32)]
    lib.jade_last_error.restype = C.c_char_p
    return lib


def ask(dbg, combo):
    mode = C.c_uint32(0xdeadbeef)
    rc = dbg.jade_debug_shade_mode_host(*combo, C.byref(mode))
    return rc, mode.value, (dbg.jade_last_error() or b"").decode()


def test_the_table_and_the_rule_are_the_same_eighteen():
    assert len(ALL) == 64 and len(ACCEPTED) == 18 and len(set(ACCEPTED.values())) == 18
    assert {c for c in ALL if refusal(*c) is None} == set(ACCEPTED)
    assert set(ACCEPTED) <= set(ALL)


@pytest.mark.parametrize("combo", sorted(ACCEPTED), ids=lambda c: "-".join(map(str, c)))
def test_a_built_mode_is_accepted_with_its_bits(dbg, combo):
    rc, mode, _ = ask(dbg, combo)
    assert rc == _abi.JADE_OK and mode == ACCEPTED[combo]


@pytest.mark.parametrize("combo", sorted(set(ALL) - set(ACCEPTED)), ids=lambda c: "-".join(map(str, c)))
def test_every_other_combination_is_refused_by_the_first_check_that_applies(dbg, combo):
    rc, mode, text = ask(dbg, combo)
    assert rc == _abi.JADE_ERR_UNSUPPORTED and mode == 0xdeadbeef, "refused, and the mode left alone"
    head, word = refusal(*combo)
    assert text.split(":")[0] in ("light sampling", "bounce sampling", "direct sampling")
    assert text.split(" ")[2] == head, f"the first check that applies names {head}: {text}"
    assert word in text
    other = {"lens": "shutter", "shutter": "lens"}.get(word)
    assert other is None or other not in text, "a lens is named before a shutter, and only one of them"


def test_a_null_result_pointer_is_refused(dbg):
    assert dbg.jade_debug_shade_mode_host(0, 0, 0, 0, 0, 0, None) == _abi.JADE_ERR_INVALID


def test_mis_under_a_lens_is_refused_by_cosines_own_check(dbg):
    rc, _, text = ask(dbg, (0, 1, 0, _abi.LIGHTS_ALL, _abi.BOUNCE_COSINE, _abi.DIRECT_MIS))
    assert rc == _abi.JADE_ERR_UNSUPPORTED and "JADE_BOUNCE_COSINE" in text and "lens" in text and "JADE_DIRECT_MIS" not in text
