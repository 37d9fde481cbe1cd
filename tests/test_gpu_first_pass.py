"""The fused first pass and the shade kernels that share its record steps, held to a recording: tests/golden/first_pass.json.

shade_record and k_shade_binned begin a sample, end a sample and park a path with shared helpers (csrc/jade_shade.h); k_light and
k_light_packet (csrc/jade_light.h) share some of them and keep their own text of the rest.  The schedule tests prove that the
schedules agree with each other; this file holds each of them to the kernels as they stood BEFORE those pieces were shared.

The scene is scene_shapes.base() - sky, an emitter, a mirror box, jade, glass and a diffuse floor: every branch of the first pass's
advance step and both kinds of hand-over (untouched, parked at a vertex) run - at 40 x 36, neither side a multiple of the 16-pixel tile, so
that the samples of out-of-image pixels are skipped.  The switches are read once per process, so every schedule renders in a fresh child
process, each in two ways: one render of 6 spp, and begin / step(2) / step(1) / step(3) / flush, where records are carried over between
the steps.  A child renders 2 x 8640 pixel-samples.

The fixture holds, per (schedule, way), the sha256 of the float frame and every integer counter of jade_stats.  It was recorded with the
parent commit's library, twice, and the two recordings were the same in every entry; the test asserts equality.  To record:

    python tests/test_gpu_first_pass.py record OUT.json     (on the MI355X; twice, and compare the two files)

A 6-spp render takes 8 records per pixel by itself, so "RECORDS_PER_PIXEL=8" (the issue's case for records beyond a pixel's first,
rec_m > 0) renders what "default" renders; "RECORDS_PER_PIXEL=1" is here for the other side, rec_m == 0 for every record."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "first_pass.json")
WIDTH, HEIGHT, SPP = 40, 36, 6
STEPS = (2, 1, 3)
SCHEDULES = {
    "default": {},
    "LIGHT_PACKET=0": {"JADE_LIGHT_PACKET": "0"},                         # k_light: one lane per ray
    "PACKET_BUDGET=3": {"JADE_PACKET_BUDGET": "3"},                       # packets are given up: the rng_vertex restore
    "FUSED=0": {"JADE_FUSED": "0"},                                       # k_shade_lean + k_shade_binned
    "FUSED=0 SHADE_BINNED=0": {"JADE_FUSED": "0", "JADE_SHADE_BINNED": "0"},  # k_shade_lean + k_shade
    "SHADE_SPLIT=0": {"JADE_SHADE_SPLIT": "0"},                           # the full kernel alone
    "RECORDS_PER_PIXEL=8": {"JADE_RECORDS_PER_PIXEL": "8"},
    "RECORDS_PER_PIXEL=1": {"JADE_RECORDS_PER_PIXEL": "1"},
}
WAYS = ("render", "steps")
assert sum(STEPS) == SPP


# ------------------------------------------------------------------------------------------------------------------ the child --

def _entry(rgb, st, _abi):
    rgb = np.ascontiguousarray(rgb, np.float32)
    assert rgb.shape == (HEIGHT, WIDTH, 3)
    counters = {n: int(getattr(st, n)) for n, t in _abi.Stats._fields_ if t is ctypes.c_uint64}
    return {"sha256": hashlib.sha256(rgb.tobytes()).hexdigest(), "counters": counters}


def child():
    """Renders the frame both ways under this process's schedule; one JSON object on the last line of stdout."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import scene_shapes
    from jaderaytracerendering_amd import _abi, backend as B, host as H

    hip = B.hip()
    hs = scene_shapes.base()
    eye, cam = H.camera_orbit(5.0, 20.0, 30.0)   # scene_shapes.params' camera
    p = B.make_params(WIDTH, HEIGHT, SPP, eye, cam)
    out = {}
    with hip.scene(hs) as sc:
        rgb, _, st = sc.render(p, want_bgr8=False)
        out["render"] = _entry(rgb, st, _abi)
        sc.begin(p)
        st = _abi.Stats()
        for n in STEPS:
            sc.step(n, st)
        sc.flush(st)
        rgb, _ = sc.resolve(want_bgr8=False)
        out["steps"] = _entry(rgb, st, _abi)
    print(json.dumps(out))


def run_child(schedule):
    env = {k: v for k, v in os.environ.items() if not k.startswith("JADE_")}
    env.update(SCHEDULES[schedule])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (schedule, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


if __name__ == "__main__":
    if sys.argv[1:] == ["child"]:
        child()
    elif len(sys.argv) == 3 and sys.argv[1] == "record":
        rec = {schedule: run_child(schedule) for schedule in SCHEDULES}
        with open(sys.argv[2], "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
            f.write("\n")
        print(f"recorded {sum(len(v) for v in rec.values())} entries to {sys.argv[2]}")
    else:
        raise SystemExit(__doc__)
    raise SystemExit(0)


# ------------------------------------------------------------------------------------------------------------------ the tests --
pytestmark = pytest.mark.gpu

with open(FIXTURE) as _f:
    RECORDED = json.load(_f)

_children = {}


def rendered(schedule):
    if schedule not in _children:
        _children[schedule] = run_child(schedule)
    return _children[schedule]


def test_the_fixture_holds_every_schedule_and_ran_what_it_is_for():
    assert sorted(RECORDED) == sorted(SCHEDULES)
    for schedule in SCHEDULES:
        assert sorted(RECORDED[schedule]) == sorted(WAYS), schedule
    # one frame, however it is scheduled or stepped
    assert len({RECORDED[s][w]["sha256"] for s in SCHEDULES for w in WAYS}) == 1
    inline = {s: RECORDED[s]["render"]["counters"]["rays_inline"] for s in SCHEDULES}
    assert inline["default"] > 0, "the fused first pass traced nothing"
    assert inline["PACKET_BUDGET=3"] < inline["default"], "no packet was given up under a budget of 3 records"
    assert inline["LIGHT_PACKET=0"] > 0 and inline["FUSED=0"] == 0 and inline["FUSED=0 SHADE_BINNED=0"] == 0
    for w in WAYS:
        assert RECORDED["RECORDS_PER_PIXEL=8"][w] == RECORDED["default"][w]


@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_schedule_renders_the_recorded_frame_and_counters(hip, schedule, way):
    got, want = rendered(schedule)[way], RECORDED[schedule][way]
    print(f"{schedule}, {way}: sha256 {got['sha256']} (recorded {want['sha256']})")
    assert got["counters"] == want["counters"]
    assert got["sha256"] == want["sha256"]
