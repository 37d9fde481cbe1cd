"""Every render mode the module builds, under three shading schedules, held to a recording: tests/golden/shade_modes.json.

The 36 modes are {reference, importance, mixture} environment sampling x {pinhole, lens, shutter, shutter+lens, one-light, cosine,
cosine+one-light, MIS, MIS+one-light, passes, passes+cosine, passes+MIS}: every row of JADE_SHADE_MODES_BUILT (csrc/jade_runtime.h), which
this module reads and holds its table to (include/jade_bvh.h; tests/test_shade_modes_cpu.py states which combinations are built and which
are refused).  Each is rendered through the public ABI on spec_scenes' two_lamps scene under the textured sky - a jade cube (mirror and
sub-surface), two lamps, a diffuse floor - at 32 x 32, 4 spp, under the default schedule, under JADE_FUSED=0 (the lean kernel and the
split hand-over run) and under JADE_SHADE_SPLIT=0 (the full kernel alone over the list).  The switches are read once per process, so every
schedule renders in a fresh child process: three children per session, each rendering all 36 modes on one scene handle.

The fixture holds, per (mode, schedule), the sha256 of the float frame and every integer counter of jade_stats; for a mode that keeps
passes also the sha256 of the fifteen pass planes as Scene.passes() returns them, in index order.  The first 18 modes (reference and
importance sampling, without passes) were recorded with the kernels as they stood BEFORE the shade kernels were folded into one family
indexed by the mode.  All 36 were recorded with the kernels as they stood BEFORE that family took its mode as one mask and its arguments
as one bundle, and the 54 entries of the first recording came out the same.  Each recording was made twice, and the two were the same in
every entry; the test asserts equality, so that either change is held to the renders of the code it replaced.  To record:

    python tests/test_gpu_shade_modes.py record OUT.json     (on the MI355X; twice, and compare the two files)

Each child also asks for a combination the module refuses (a lens with one-light sampling) after its 36 renders, and then renders the
parity mode again on the same handle: a refusal must leave the scene usable, and that frame is the fixture's "reference/pinhole" entry."""
import ctypes
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "shade_modes.json")
SIZE, SPP = 32, 4
LENS = (0.1, 2.8)
SHUTTER_CLOSE = (2.8, 24.0, 11.0)   # camera_orbit of the closing pose; the opening pose is the render's (2.8, 20, 10)
SHUTTER_INTERVAL = (0.25, 1.0)

#            lens   shutter one-light cosine MIS    passes
CAMERAS = {
    "pinhole":          (False, False, False, False, False, False),
    "lens":             (True,  False, False, False, False, False),
    "shutter":          (False, True,  False, False, False, False),
    "shutter+lens":     (True,  True,  False, False, False, False),
    "one-light":        (False, False, True,  False, False, False),
    "cosine":           (False, False, False, True,  False, False),
    "cosine+one-light": (False, False, True,  True,  False, False),
    "MIS":              (False, False, False, True,  True,  False),
    "MIS+one-light":    (False, False, True,  True,  True,  False),
}
PASSES = {
    "passes":           (False, False, False, False, False, True),
    "passes+cosine":    (False, False, False, True,  False, True),
    "passes+MIS":       (False, False, False, True,  True,  True),
}
ENVS = ("reference", "importance", "mixture")
# in the order a child renders them: the 18 modes of the first recording as it rendered them, then the mixture, then the passes
MODES = {f"{env}/{name}": (env,) + flags for env in ENVS[:2] for name, flags in CAMERAS.items()}
MODES.update({f"mixture/{name}": ("mixture",) + flags for name, flags in CAMERAS.items()})
MODES.update({f"{env}/{name}": (env,) + flags for env in ENVS for name, flags in PASSES.items()})
SCHEDULES = {"default": {}, "FUSED=0": {"JADE_FUSED": "0"}, "SHADE_SPLIT=0": {"JADE_SHADE_SPLIT": "0"}}
PARITY = "reference/pinhole"


def built_masks():
    """ShadeMode's bits and the masks JADE_SHADE_MODES_BUILT lists (its rows x JADE_SHADE_MODE_BOTH_ENV's columns), read from csrc/jade_runtime.h."""
    with open(os.path.join(ROOT, "jaderaytracerendering_amd", "csrc", "jade_runtime.h")) as f:
        text = f.read().replace("\\\n", " ")
    bit = {name: int(v) for name, v in re.findall(r"^\s*(SM_[A-Z]+) = (\d+)u,", text, re.M)}
    mask = lambda expr: sum(bit[t.strip()] for t in expr.split("|") if t.strip() not in ("", "0u"))
    rows = re.findall(r"JADE_SHADE_MODE_BOTH_ENV\(X, ([^)]*)\)", re.search(r"#define JADE_SHADE_MODES_BUILT\(X\)(.*)", text).group(1))
    cols = re.findall(r"X\(\(m\)([^)]*)\)", re.search(r"#define JADE_SHADE_MODE_BOTH_ENV\(X, m\)(.*)", text).group(1))
    return bit, [mask(r) | mask(c) for r in rows for c in cols]


def mask_of(bit, env, lens, shutter, one_light, cosine, mis, passes):
    m = {"reference": 0, "importance": bit["SM_ENVIS"], "mixture": bit["SM_ENVIS"] | bit["SM_ENVMIX"]}[env]
    for on, name in ((lens, "SM_LENS"), (shutter, "SM_SHUTTER"), (one_light, "SM_LIGHTS"), (cosine, "SM_COSINE"), (mis, "SM_MIS"), (passes, "SM_PASSES")):
        m |= bit[name] if on else 0
    return m


_bit, _built = built_masks()
assert len(MODES) == len(_built) == 36 and PARITY in MODES
assert sorted(mask_of(_bit, *flags) for flags in MODES.values()) == sorted(_built), "the table is the list of built modes, mode for mode"


# ------------------------------------------------------------------------------------------------------------------ the child --

def _set_mode(sc, H, _abi, lens, shutter, one_light, cosine, mis, passes=False):
    sc.set_lens(*LENS) if lens else sc.set_lens(None)
    if shutter:
        eye_c, cam_c = H.camera_orbit(*SHUTTER_CLOSE)
        sc.set_shutter(eye_c, cam_c, *SHUTTER_INTERVAL)
    else:
        sc.set_shutter(None)
    sc.set_light_sampling(_abi.LIGHTS_ONE if one_light else _abi.LIGHTS_ALL)
    sc.set_bounce_sampling(_abi.BOUNCE_COSINE if cosine else _abi.BOUNCE_UNIFORM)
    sc.set_direct_sampling(_abi.DIRECT_MIS if mis else _abi.DIRECT_RAYS)
    sc.set_passes(passes)


def _entry(rgb, st, _abi):
    rgb = np.ascontiguousarray(rgb, np.float32)
    assert rgb.shape == (SIZE, SIZE, 3)
    counters = {n: int(getattr(st, n)) for n, t in _abi.Stats._fields_ if t is ctypes.c_uint64}
    return {"sha256": hashlib.sha256(rgb.tobytes()).hexdigest(), "counters": counters}


def child():
    """Renders every mode under this process's schedule; one JSON object on the last line of stdout."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import spec_scenes as SP
    from jaderaytracerendering_amd import _abi, backend as B, host as H

    hip = B.hip()
    hs = SP.build("two_lamps", sky=True)
    eye, cam = H.camera_orbit(2.8, 20.0, 10.0)
    out = {}
    with hip.scene(hs) as sc:
        env_sampling = {"reference": _abi.ENV_REFERENCE, "importance": _abi.ENV_IMPORTANCE, "mixture": _abi.ENV_MIXTURE}
        for name, (env, *flags) in MODES.items():
            _set_mode(sc, H, _abi, *flags)
            p = B.make_params(SIZE, SIZE, SPP, eye, cam, env_sampling=env_sampling[env])
            rgb, _, st = sc.render(p, want_bgr8=False)
            out[name] = _entry(rgb, st, _abi)
            if flags[-1]:  # the pass planes of the render just made, in index order
                planes = sc.passes()
                assert list(planes) == list(_abi.PASS_NAMES)
                stack = np.ascontiguousarray(np.stack(list(planes.values())), np.float32)
                assert stack.shape == (_abi.PASS_COUNT, SIZE, SIZE, 3)
                out[name]["passes_sha256"] = hashlib.sha256(stack.tobytes()).hexdigest()
        # a refused combination, asked for while the last render (mixture / passes + MIS) is still the scene's ...
        _set_mode(sc, H, _abi, True, False, True, False, False)
        p = B.make_params(SIZE, SIZE, SPP, eye, cam)
        try:
            sc.begin(p)
            out["refusal"] = None
        except B.JadeError as e:
            out["refusal"] = {"code": e.code, "text": str(e)}
        # ... then the parity mode on the same handle
        _set_mode(sc, H, _abi, False, False, False, False, False)
        rgb, _, st = sc.render(p, want_bgr8=False)
        out["after refusal"] = _entry(rgb, st, _abi)
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
        rec = {}
        for schedule in SCHEDULES:
            got = run_child(schedule)
            assert got["refusal"] and got["after refusal"] == got[PARITY], (schedule, got["refusal"])
            rec[schedule] = {name: got[name] for name in MODES}
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


def test_the_fixture_holds_every_mode_under_every_schedule():
    assert sorted(RECORDED) == sorted(SCHEDULES)
    for schedule in SCHEDULES:
        assert sorted(RECORDED[schedule]) == sorted(MODES), schedule
    frames = {RECORDED["default"][m]["sha256"] for m in MODES}
    assert len(frames) == len({flags[:-1] for flags in MODES.values()}), "keeping passes changes no bit of a frame; every other mode has a frame of its own"
    for schedule in SCHEDULES:
        for mode, flags in MODES.items():
            assert ("passes_sha256" in RECORDED[schedule][mode]) == flags[-1], (schedule, mode)


@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("mode", list(MODES))
def test_mode_renders_the_recorded_frame_and_counters(hip, mode, schedule):
    got, want = rendered(schedule)[mode], RECORDED[schedule][mode]
    print(f"{mode} under {schedule}: sha256 {got['sha256']} (recorded {want['sha256']})")
    assert got["counters"] == want["counters"]
    assert got["sha256"] == want["sha256"]
    assert got.get("passes_sha256") == want.get("passes_sha256")


@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_a_refused_combination_leaves_the_scene_usable(hip, schedule):
    from jaderaytracerendering_amd import _abi
    got = rendered(schedule)
    assert got["refusal"] is not None, "a lens with one-light sampling is refused"
    assert got["refusal"]["code"] == _abi.JADE_ERR_UNSUPPORTED and "JADE_LIGHTS_ONE" in got["refusal"]["text"] and "lens" in got["refusal"]["text"]
    assert got["after refusal"] == RECORDED[schedule][PARITY]
