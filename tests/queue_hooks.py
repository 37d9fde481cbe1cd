"""What tests/test_gpu_ray_records.py and tests/test_gpu_trace_chunks.py share: the three small frames, a render under a set of development
switches (Tunables reads the environment once, at jade_scene_create: the scene is made inside the setting), jade_debug_ray_record_use, and
"the same frame": every float of the radiance, every byte, every counter of conftest.counters."""
import contextlib
import ctypes as C
import os

import numpy as np

from conftest import B, config_scene, counters
from jaderaytracerendering_amd import _abi, host as H

# tiny / tinyjade at 48 x 32 (3 x 2 whole tiles, 1536 pixels) and 4 spp: 6144 records, several 256-thread blocks of k_trace; the jade branch
# of tinyjade fills every slot of a record.  C2 at 64 x 48 and 2 spp with an ordered queue: the 70 k-triangle statue, queue POSITIONS sorted.
FRAMES = {
    "tiny": ("tiny", 48, 32, 4, {}),
    "tinyjade": ("tinyjade", 48, 32, 4, {}),
    "C2": ("C2", 64, 48, 2, {"JADE_SORT": "1", "JADE_SORT_MIN": "64"}),
    # 121 pixels of one tile with ONE record each, whatever the samples: no pass queues more than 121 x 4 rays (single-wave passes,
    # tests/test_gpu_ray_records.py)
    "tinyjade-11x11": ("tinyjade", 11, 11, 8, {"JADE_RECORDS_PER_PIXEL": "1"}),
    "C2-11x11": ("C2", 11, 11, 4, {"JADE_RECORDS_PER_PIXEL": "1"}),
}
LENS = (0.02, 0.45)  # tinyjade: the statuette sits 0.40 - 0.48 deep (tests/render_helpers.py, SCHED_LENS)


def frame(name):
    config, w, h, spp, env = FRAMES[name]
    hs, cfg = config_scene(config)
    p = B.params_from_config(cfg, spp=spp)
    p.width, p.height = w, h
    return hs, p, env


def shutter_close(p):
    """tests/test_gpu_shutter.py's move for tinyjade: a turntable step of 3 degrees about the orbit's centre and a small truck."""
    eye, cam = np.array(p.eye[:], np.float32), np.array(p.camera[:], np.float32)
    return H.camera_move(eye, cam, truck=(0.004, -0.002, 0.0), orbit_deg=3.0, pivot=(0.26, -1.28, 0.0))


@contextlib.contextmanager
def environment(env):
    before = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        yield
    finally:
        for k, v in before.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def record_use(be, sc):
    """jade_debug_ray_record_use (libjade_hip_debug.so): rays k_trace took since jade_render_begin from queue positions (below the record
    boundary, at or beyond it); None on a library without the entry point."""
    fn = getattr(be.lib, "jade_debug_ray_record_use", None)
    if fn is None:
        return None
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
    out = (C.c_int64 * 2)()
    be.check(fn(sc._h, out))
    return int(out[0]), int(out[1])


def render(be, name, env, walk=_abi.WALK_REFERENCE, prepare=None, renders=1, steps=None):
    """The frame `name` under its own switches + `env`: (rgb, bgr, stats, record use) of the last of `renders` renders on one handle.
    prepare(sc, p): a lens, a shutter.  steps: the samples of progressive steps (then a flush) instead of one call."""
    hs, p, base = frame(name)
    q = type(p).from_buffer_copy(p)
    q.walk = walk
    out = None
    with environment({**base, **env}), be.scene(hs) as sc:
        if prepare:
            prepare(sc, q)
        for _ in range(renders):
            if steps:
                st = _abi.Stats()
                sc.begin(q)
                for n in steps:
                    sc.step(n, st)
                sc.flush(st)
                out = sc.resolve() + (st,)
            else:
                out = sc.render(q)
            out = out + (record_use(be, sc),)
    return out


def assert_same_frame(got, ref, what, keys=None):
    assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)), f"{what}: radiance differs in {int((got[0].view(np.uint32) != ref[0].view(np.uint32)).sum())} floats"
    assert np.array_equal(got[1], ref[1]), f"{what}: bytes differ"
    a, b = counters(got[2]), counters(ref[2])
    if keys is not None:
        a, b = {k: a[k] for k in keys}, {k: b[k] for k in keys}
    assert a == b, f"{what}: {a} != {b}"
