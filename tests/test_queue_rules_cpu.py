"""The two sizing rules of k_trace's refill, without a GPU ("Ray records" and "k_trace").

ray_record_cap (jade_runtime.h): how many positions of the ray queue have a 48-byte ray record - setup_state sizes b_rayq and sets
PathState.rayq_cap from it.  trace_chunk_for: how many rays a wave of k_trace claims per queue atomic - launch_trace passes it to the kernel,
and trace_body restates it on the device for batched passes.  libjade_hip_debug.so exports both as they are (no HIP call, no environment);
here each is held against a numpy statement over a table of slot and ray counts, the two test hooks (JADE_RAYQ_CAP, JADE_TRACE_CHUNK_RAYS:
tests/test_gpu_ray_records.py, tests/test_gpu_trace_chunks.py) included."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT

CHUNK_MAX = 512  # JADE_TRACE_CHUNK (jade_device.h)


@pytest.fixture(scope="module")
def dbg():
    path = os.path.join(ROOT, "jaderaytracerendering_amd", "lib", "libjade_hip_debug.so")
    assert os.path.exists(path), "libjade_hip_debug.so missing: run `make hipvariants` (or __graft_entry__.build())"
    lib = C.CDLL(path)
    lib.jade_debug_ray_record_cap_host.restype = C.c_int64
    lib.jade_debug_ray_record_cap_host.argtypes = [C.c_uint64, C.c_int32, C.c_int64]
    lib.jade_debug_trace_chunk_host.restype = C.c_uint32
    lib.jade_debug_trace_chunk_host.argtypes = [C.c_uint32, C.c_uint64, C.c_uint32]
    return lib


# ------------------------------------------------------------------------------------------------------------- the record boundary --

def cap_rule(slots):
    """The statement: an eighth of all slots (rounded up), but every slot of a queue of up to 2^22; never more than there are slots."""
    slots = np.asarray(slots, np.uint64)
    eighth = (slots + np.uint64(7)) // np.uint64(8)
    return np.minimum(np.maximum(eighth, np.minimum(slots, np.uint64(1 << 22))), slots)


SLOTS = [0, 1, 2, 7, 8, 9, 4095, (1 << 22) - 1, 1 << 22, (1 << 22) + 1, (1 << 25) - 8, (1 << 25) - 7, (1 << 25) - 1, 1 << 25, (1 << 25) + 1,
         (1 << 25) + 8, 3 * (1 << 25) + 5, (1 << 32) - 1]


def test_cap_rule_values_at_the_edges():
    """The statement itself, in plain numbers: all slots up to 2^22, then 2^22 flat until an eighth overtakes it at 2^25."""
    want = {0: 0, 1: 1, (1 << 22) - 1: (1 << 22) - 1, 1 << 22: 1 << 22, (1 << 22) + 1: 1 << 22, (1 << 25) - 8: 1 << 22, (1 << 25) - 7: 1 << 22,
            1 << 25: 1 << 22, (1 << 25) + 1: (1 << 22) + 1, (1 << 25) + 8: (1 << 22) + 1, (1 << 25) + 9: (1 << 22) + 2, (1 << 32) - 1: 1 << 29}
    for slots, cap in want.items():
        assert int(cap_rule(slots)) == cap, slots


def test_ray_record_cap_is_the_rule(dbg):
    want = cap_rule(SLOTS)
    for slots, w in zip(SLOTS, want):
        got = dbg.jade_debug_ray_record_cap_host(slots, 1, 0)
        assert got == int(w), (slots, got, int(w))
        assert 0 <= got <= slots
        assert dbg.jade_debug_ray_record_cap_host(slots, 0, 0) == 0, "records switched off: none"
        assert dbg.jade_debug_ray_record_cap_host(slots, 0, 5) == 0, "... whatever the hook says"
        for unset in (0, -1, -(1 << 40)):
            assert dbg.jade_debug_ray_record_cap_host(slots, 1, unset) == int(w), "a hook of 0 or less means the rule"


def test_the_cap_hook_only_lowers(dbg):
    for slots, w in zip(SLOTS, cap_rule(SLOTS)):
        w = int(w)
        hooks = {1, 63, 64, 65, 100, 4096, w - 1, w, w + 1, 2 * w + 3, slots, slots + 1, 1 << 40}
        for hook in sorted(h for h in hooks if h > 0):
            got = dbg.jade_debug_ray_record_cap_host(slots, 1, hook)
            assert got == min(w, hook), (slots, hook, got)
            assert got <= w and got <= slots


def test_ray_record_cap_over_a_random_table(dbg):
    rng = np.random.default_rng(22)
    slots = np.concatenate([rng.integers(0, 1 << 12, 200), rng.integers(0, 1 << 26, 400), rng.integers(0, 1 << 32, 400)]).astype(np.uint64)
    hooks = np.where(rng.random(len(slots)) < 0.5, 0, rng.integers(1, 1 << 27, len(slots)))
    want = cap_rule(slots)
    for s, h, w in zip(slots.tolist(), hooks.tolist(), want.tolist()):
        assert dbg.jade_debug_ray_record_cap_host(s, 1, h) == (min(w, h) if h > 0 else w), (s, h)


# -------------------------------------------------------------------------------------------------------------------- claim chunks --

def chunk_rule(n_rays, waves):
    """The statement: aim at 8 claims per wave - n_rays / (waves x 64 x 8) whole groups of 64, at least one group, at most 512 rays."""
    per = np.asarray(n_rays, np.uint64) // (np.asarray(waves, np.uint64) * np.uint64(512))
    return np.clip(per, 1, CHUNK_MAX // 64) * np.uint64(64)


WAVES = (4, 1024, 5120)
IGNORED_HOOKS = (0, 1, 32, 63, 65, 100, 127, 129, 513, 576, 1024, 4096, (1 << 32) - 64, (1 << 32) - 1)
TAKEN_HOOKS = (64, 128, 192, 256, 320, 384, 448, 512)  # every multiple of 64 in 64..512; 64, 128, 256 and 512 are the ones the GPU tests run


def _ray_counts(waves):
    """0, 1, and both sides of every step of the rule: per = k for k = 1 .. 8 and past the ceiling."""
    n = {0, 1, 63, 64, 65}
    for k in (1, 2, 3, 4, 5, 6, 7, 8, 9, 16):
        edge = waves * 512 * k
        n |= {edge - 1, edge, edge + 1}
    n |= {(1 << 32) - 1}
    return sorted(v for v in n if 0 <= v < (1 << 32))


def test_chunk_rule_values_at_the_edges():
    for waves in WAVES:
        assert int(chunk_rule(0, waves)) == 64 and int(chunk_rule(1, waves)) == 64
        assert int(chunk_rule(waves * 512 - 1, waves)) == 64 and int(chunk_rule(waves * 512, waves)) == 64
        for k, want in ((2, 128), (4, 256), (8, 512), (16, 512)):
            assert int(chunk_rule(waves * 512 * k - 1, waves)) == min(64 * (k - 1), 512)
            assert int(chunk_rule(waves * 512 * k, waves)) == want
    assert int(chunk_rule(16 * 5120 * 64, 5120)) == 128  # (the issue's "16 x waves x 64 rays": the first launch that leaves 64)


@pytest.mark.parametrize("waves", WAVES)
def test_trace_chunk_is_the_rule(dbg, waves):
    for n in _ray_counts(waves):
        want = int(chunk_rule(n, waves))
        got = dbg.jade_debug_trace_chunk_host(n, waves, 0)
        assert got == want, (n, waves, got, want)
        assert got % 64 == 0 and 64 <= got <= CHUNK_MAX
        for hook in IGNORED_HOOKS:
            assert dbg.jade_debug_trace_chunk_host(n, waves, hook) == want, (n, waves, hook)
        for hook in TAKEN_HOOKS:
            assert dbg.jade_debug_trace_chunk_host(n, waves, hook) == hook, (n, waves, hook)


def test_trace_chunk_over_a_random_table(dbg):
    rng = np.random.default_rng(23)
    n = rng.integers(0, 1 << 32, 1000).astype(np.uint64)
    n[:300] >>= rng.integers(0, 24, 300).astype(np.uint64)
    waves = rng.choice([1, 4, 24, 1024, 4096, 5120], 1000)
    want = chunk_rule(n, waves)
    for a, w, c in zip(n.tolist(), waves.tolist(), want.tolist()):
        assert dbg.jade_debug_trace_chunk_host(a, w, 0) == c, (a, w)
