"""The seams every render mode is held to, written once: CASES has one entry per mode and the check_* functions ask each entry the
same questions.  tests/test_gpu_mode_seams.py runs every check for every case on the device; tests/test_mode_seams_cpu.py runs them
against a stand-in that can be made wrong.

A check takes the backend, the case and - where it compares with it - the case's reference render, made once by reference().  Every
check fails with AssertionError and nothing else, so that a stand-in's fault can be told from a mistake in the check.

Adding a render mode: one entry in CASES.  What is particular to the mode - its draw against its spec, its anchors,
its work and memory, its integral - goes into the mode's own test file."""
import subprocess
from dataclasses import dataclass, field
from typing import Callable, Optional

import numpy as np

import lamp_scenes
from camera_cases import quad_scene, tinyjade
from conftest import ORACLE_LIB, counters
from jaderaytracerendering_amd import _abi, backend as B
from render_helpers import CLI, SCHED_LENS, all_counters, not_walk, same_bits, sum_of_shares, with_params

ONE, ALL = _abi.LIGHTS_ONE, _abi.LIGHTS_ALL
COS, UNI = _abi.BOUNCE_COSINE, _abi.BOUNCE_UNIFORM
MIS, RAYS = _abi.DIRECT_MIS, _abi.DIRECT_RAYS
WALKS = (_abi.WALK_REFERENCE, _abi.WALK_EARLY_EXIT, _abi.WALK_EARLY_EXIT_CACHED)

# ------------------------------------------------------------------------------------------------------------------ schedules --
# Environment switches, read once at jade_scene_create.  Every case runs the common list: records per pixel, the unfused first pass, the
# serial shade and trace, ordered queues with the keys from either kernel, and switches of kernels the sampling modes do not run.
COMMON_SCHEDULES = [
    dict(JADE_RECORDS_PER_PIXEL="1"), dict(JADE_FUSED="0"), dict(JADE_SHADE_SPLIT="0", JADE_BATCH="0", JADE_RAY_RECORDS="0"),
    dict(JADE_SORT="1", JADE_SORT_MIN="64"), dict(JADE_SORT="1", JADE_SORT_MIN="64", JADE_SORT_KEYS_KERNEL="1"),
    dict(JADE_SHADE_BINNED="1", JADE_TAIL="1"), dict(JADE_TAIL="0", JADE_LIGHT_PACKET="0"),
]
# ... and the camera modes each switch by itself: most are switches of kernels that have no lens or shutter form, and change nothing
CAMERA_SCHEDULES = [
    dict(JADE_BATCH="0"), dict(JADE_BATCH="1"), dict(JADE_SHADE_SPLIT="0"), dict(JADE_SHADE_SPLIT="1"), dict(JADE_RAY_RECORDS="0"),
    dict(JADE_RAY_RECORDS="1"), dict(JADE_RECORDS_PER_PIXEL="64"), dict(JADE_FUSED="1"), dict(JADE_LIGHT_PACKET="0"), dict(JADE_LIGHT_PACKET="1"),
    dict(JADE_TAIL="0"), dict(JADE_TAIL="1"), dict(JADE_SHADE_BINNED="0"), dict(JADE_SHADE_BINNED="1"),
    dict(JADE_FUSED="0", JADE_TAIL="0", JADE_SHADE_BINNED="1", JADE_LIGHT_PACKET="0"),
]


def schedule_id(env):
    return ",".join(f"{k[5:]}={v}" for k, v in env.items())


# ------------------------------------------------------------------------------------------------------------------ invariants --

def camera_invariants(st):
    """A lens or a shutter: every camera ray goes through k_trace, one per sample; the fused first pass and the tail kernel have no such
    form."""
    assert st.rays_inline == 0 and st.tail_launches == 0 and st.rays_tail == 0 and st.rays_primary == st.samples, all_counters(st)


def sampling_invariants(st):
    """One-light, cosine, MIS: the fused first pass stays, the tail kernel does not run."""
    assert st.rays_inline > 0 and st.tail_launches == 0, (st.rays_inline, st.tail_launches)


def no_tail_kernel(st):
    assert st.tail_launches == 0, st.tail_launches


# `rays_inline > 0` holds if and only if the first pass is fused, and these two environments switch the fused first pass off
# (jade_runtime.h: fused = shade_split && !JADE_FUSED=0).  Applied to every schedule for the first time here, sampling_invariants failed
# under both in all three sampling cases on the MI355X (mode_seams.py, sampling_invariants: AssertionError); the parents asserted no
# invariant under a schedule.  Case.schedules_without_first_pass names the environments that are held to no_tail_kernel instead.
UNFUSED_SCHEDULES = [dict(JADE_FUSED="0"), dict(JADE_SHADE_SPLIT="0", JADE_BATCH="0", JADE_RAY_RECORDS="0")]


# ------------------------------------------------------------------------------------------------------------------------ cases --

@dataclass
class Case:
    name: str
    scene: Callable                    # () -> the host scene
    params: Callable                   # () -> the render parameters
    apply: Callable                    # (sc): puts the mode on a handle
    switch: Optional[Callable]         # (sc): what a render in progress is switched to before its flush - and ignores
    steps: tuple                       # (number of steps, samples per step)
    shares: int                        # tile shares that must assemble to the frame
    invariants: Callable               # (stats): what holds of every render's statistics, a share's included
    small_scene: Callable              # () -> a scene for the checks that render nothing
    oracle_calls: Callable             # (so) -> (the setter's call, the getter's call): the oracle refuses both
    multi_unequal: list                # [(s1) -> None]: settings of the second handle that jade_render_multi refuses ...
    multi_words: str                   # ... with this in the text
    multi_unset: Optional[Callable] = None   # (sc): on both handles, jade_render_multi accepts the pair again
    extra_schedules: list = field(default_factory=list)
    rpp_default: Optional[int] = None  # Q_RECORDS_PER_PIXEL where JADE_RECORDS_PER_PIXEL is not set (None: not asserted)
    knob: Optional[tuple] = None       # sampling modes: (the handle's property, its setter, the mode's value)
    usable: list = field(default_factory=list)   # check_refusal_leaves_the_handle_usable's steps
    cli: Optional[dict] = None         # check_command_line's flags and texts
    schedules_without_first_pass: list = field(default_factory=list)   # environments held to no_tail_kernel alone (UNFUSED_SCHEDULES)


def _close():
    return tinyjade(64)[2]


def _other_eye():
    eye = _close()[0].copy()
    eye[0] = np.nextafter(eye[0], np.float32(10))
    return eye


def _lamp_pose():
    p = lamp_scenes.params()
    return np.array(p.eye[:], np.float32), np.array(p.camera[:], np.float32)


def _camera_case(name, apply, switch, oracle_calls, multi_unequal, multi_words, multi_unset=None):
    return Case(name=name, scene=lambda: tinyjade(64)[0], params=lambda: tinyjade(64)[1], apply=apply, switch=switch, steps=(4, 16), shares=3,
                invariants=camera_invariants, small_scene=quad_scene, oracle_calls=oracle_calls, multi_unequal=multi_unequal,
                multi_words=multi_words, multi_unset=multi_unset, extra_schedules=CAMERA_SCHEDULES)


def _sampling_case(name, prop, setter, value, default, token, noun, cli, before=None, usable=None):
    """before: what the mode needs on the handle beside its own setter (MIS: cosine bounces)."""
    def apply(sc):
        if before:
            before(sc)
        getattr(sc, setter)(value)

    def usable_steps():
        # a lens, then a shutter, is refused by name and leaves the handle usable; ... and with the default mode both still render
        return [("do", apply), ("do", lambda sc: sc.set_lens(0.05, 4.0)), ("refused", "begin", (token, "lens")),
                ("do", lambda sc: (sc.set_lens(0.0), sc.set_shutter(*_lamp_pose()))), ("refused", "render", (token, "shutter")),
                ("do", lambda sc: sc.set_shutter(None)), ("reference",),
                ("do", lambda sc: (getattr(sc, setter)(default), sc.set_lens(0.05, 4.0))), ("finite",)]

    return Case(name=name, scene=lambda: lamp_scenes.lamp_scene("lamp"), params=lamp_scenes.params, apply=apply,
                switch=lambda sc: getattr(sc, setter)(default), steps=(3, 2), shares=2, invariants=sampling_invariants,
                small_scene=lambda: lamp_scenes.lamp_scene("lamp1"),
                oracle_calls=lambda so: (lambda: getattr(so, setter)(value), lambda: getattr(so, prop)),
                multi_unequal=[lambda s1: getattr(s1, setter)(default)], multi_words=noun, rpp_default=8,
                knob=(prop, setter, value), usable=usable if usable is not None else usable_steps(), cli=cli,
                schedules_without_first_pass=UNFUSED_SCHEDULES)


_CLI_BASE = ["--config", "tiny", "--width", "48", "--height", "40", "--spp", "4"]
_ON_THE_ORACLE = ["--backend", ORACLE_LIB]

_OTHER_SHUTTERS = [lambda s1: s1.set_shutter(_other_eye(), _close()[1]), lambda s1: s1.set_shutter(*_close(), 0.0, 0.5),
                   lambda s1: s1.set_shutter(None)]
CASES = [
    _camera_case("lens", apply=lambda sc: sc.set_lens(*SCHED_LENS), switch=lambda sc: sc.set_lens(None),
                 oracle_calls=lambda so: (lambda: so.set_lens(0.1, 2.0), lambda: so.lens()),
                 multi_unequal=[lambda s1: s1.set_lens(SCHED_LENS[0], 0.5), lambda s1: s1.set_lens(0.03, SCHED_LENS[1]), lambda s1: s1.set_lens(None)],
                 multi_words="lenses"),
    _camera_case("shutter", apply=lambda sc: sc.set_shutter(*_close()), switch=lambda sc: sc.set_shutter(None),
                 oracle_calls=lambda so: (lambda: so.set_shutter((0, 0, 1), np.eye(4, dtype=np.float32).ravel()), lambda: so.shutter()),
                 multi_unequal=_OTHER_SHUTTERS, multi_words="shutters", multi_unset=lambda sc: sc.set_shutter(None)),
    _camera_case("shutter+lens", apply=lambda sc: (sc.set_lens(*SCHED_LENS), sc.set_shutter(*_close())),
                 switch=lambda sc: (sc.set_shutter(None), sc.set_lens(None)),
                 oracle_calls=lambda so: (lambda: so.set_shutter(None), lambda: so.shutter()),
                 multi_unequal=_OTHER_SHUTTERS, multi_words="shutters", multi_unset=lambda sc: sc.set_shutter(None)),
    _sampling_case("one-light", "light_sampling", "set_light_sampling", ONE, ALL, "JADE_LIGHTS_ONE", "light sampling",
                   cli=dict(flags=["--one-light"], suffix="on hip-gfx950, one light per vertex",
                            refused=[(["--one-light"] + _ON_THE_ORACLE, ("--one-light needs the HIP backend",))])),
    _sampling_case("cosine", "bounce_sampling", "set_bounce_sampling", COS, UNI, "JADE_BOUNCE_COSINE", "bounce sampling",
                   cli=dict(flags=["--bounce", "cosine"], suffix="on hip-gfx950, cosine-weighted bounces",
                            refused=[(["--bounce", "cosine"] + _ON_THE_ORACLE, ("--bounce needs the HIP backend",)),
                                     (["--bounce", "sideways"], ("uniform or cosine",))])),
    _sampling_case("MIS", "direct_sampling", "set_direct_sampling", MIS, RAYS, "JADE_DIRECT_MIS", "direct sampling",
                   before=lambda sc: sc.set_bounce_sampling(COS),
                   # without cosine bounces the mode is refused by name; then cosine's own check of a lens
                   usable=[("do", lambda sc: sc.set_direct_sampling(MIS)), ("refused", "begin", ("JADE_DIRECT_MIS", "JADE_BOUNCE_COSINE")),
                           ("do", lambda sc: sc.set_bounce_sampling(COS)), ("reference",),
                           ("do", lambda sc: sc.set_lens(0.05, 4.0)), ("refused", "begin", ("JADE_BOUNCE_COSINE", "lens"))],
                   cli=dict(flags=["--bounce", "cosine", "--direct", "mis"], suffix="cosine-weighted bounces, emitters by multiple importance sampling",
                            refused=[(["--direct", "mis"], ("--direct mis", "--bounce cosine")), (["--direct", "sideways"], ("rays or mis",))])),
]
BY_NAME = {c.name: c for c in CASES}
SAMPLING = [c.name for c in CASES if c.knob]


def schedules(case):
    return COMMON_SCHEDULES + case.extra_schedules


# ----------------------------------------------------------------------------------------------------------------------- checks --

_refs = {}


def reference(be, case):
    """The case's reference render on a backend, (rgb, bgr, stats): made once per process and left unchanged."""
    if (be, case.name) not in _refs:
        with be.scene(case.scene()) as sc:
            case.apply(sc)
            _refs[be, case.name] = sc.render(case.params())
    return _refs[be, case.name]


def refused(call, code, words=()):
    """call() must raise JadeError(code) with every one of `words` in its text; returns the text."""
    try:
        call()
    except B.JadeError as e:
        assert e.code == code, (e.code, code, str(e))
        for w in words:
            assert w in str(e), (w, str(e))
        return str(e)
    raise AssertionError("not refused")


def _same_frame(out, ref, what):
    assert same_bits(out[0], ref[0]) and np.array_equal(out[1], ref[1]), what


def is_reference(case, out, ref, what="", invariants=None):
    """The frame in every bit and byte, every counter of COUNTER_KEYS, and the mode's invariants."""
    _same_frame(out, ref, what)
    assert counters(out[2]) == counters(ref[2]), what
    (invariants or case.invariants)(out[2])


def check_twice(be, case, ref):
    p = case.params()
    case.invariants(ref[2])
    assert ref[2].samples == p.width * p.height * p.spp
    assert np.isfinite(ref[0]).all() and ref[0].max() > 0
    with be.scene(case.scene()) as sc:
        case.apply(sc)
        out = sc.render(p)
    is_reference(case, out, ref, "twice")
    assert all_counters(out[2]) == all_counters(ref[2]), "every integer of jade_stats"


def check_walks(be, case, ref):
    """The three walks of jade_render_params.walk, the cached one twice on its handle (the second time with what the first left in the
    cache): the same frame and every counter but the two that count what a walk read."""
    for walk in WALKS:
        with be.scene(case.scene()) as sc:
            case.apply(sc)
            for _ in range(2 if walk == _abi.WALK_EARLY_EXIT_CACHED else 1):
                out = sc.render(with_params(case.params(), walk=walk))
                _same_frame(out, ref, walk)
                assert not_walk(out[2]) == not_walk(ref[2]), walk
                if walk == _abi.WALK_EARLY_EXIT_CACHED:
                    assert out[2].rays_cached <= out[2].rays_shadow + out[2].rays_env


def check_steps(be, case, ref):
    """Steps and a flush equal one call; a render in progress keeps the mode it began with."""
    n, spp = case.steps
    p = case.params()
    assert n * spp == p.spp
    with be.scene(case.scene()) as sc:
        case.apply(sc)
        sc.begin(p)
        st = _abi.Stats()
        for _ in range(n):
            sc.step(spp, st)
        if case.switch:
            case.switch(sc)
        sc.flush(st)
        rgb, bgr = sc.resolve()
    is_reference(case, (rgb, bgr, st), ref, f"{n} steps of {spp} + flush")


def check_shares(be, case, ref):
    with be.scene(case.scene()) as sc:
        case.apply(sc)
        acc, acc_b, tot = sum_of_shares(sc, case.params(), case.shares, each=case.invariants)
    assert same_bits(acc, ref[0]) and np.array_equal(acc_b, ref[1])
    assert tot == counters(ref[2])


def check_schedule(be, case, ref, env, setenv):
    """setenv(name, value) sets the environment for this check alone (read once, at jade_scene_create)."""
    for k, v in env.items():
        setenv(k, v)
    p = case.params()
    with be.scene(case.scene()) as sc:
        case.apply(sc)
        sc.begin(p)
        rpp = sc.query(_abi.Q_RECORDS_PER_PIXEL)
        out = sc.render(p)
        early = sc.render(with_params(p, walk=_abi.WALK_EARLY_EXIT))
    if "JADE_RECORDS_PER_PIXEL" in env:
        assert rpp == int(env["JADE_RECORDS_PER_PIXEL"])
    elif case.rpp_default is not None:
        assert rpp == case.rpp_default
    is_reference(case, out, ref, env, invariants=no_tail_kernel if env in case.schedules_without_first_pass else None)
    _same_frame(early, ref, (env, "early exits"))
    assert not_walk(early[2]) == not_walk(ref[2]), env


def check_unknown_value(be, case):
    prop, setter, value = case.knob
    with be.scene(case.small_scene()) as sc:
        getattr(sc, setter)(value)
        for bad in (2, -1, 255):
            refused(lambda: getattr(sc, setter)(bad), _abi.JADE_ERR_INVALID)
            assert getattr(sc, prop) == value


def check_oracle_refuses(oracle, case):
    with oracle.scene(case.small_scene()) as so:
        set_it, get_it = case.oracle_calls(so)
        refused(set_it, _abi.JADE_ERR_UNSUPPORTED)
        try:
            get_it()
        except B.JadeError:
            return
    raise AssertionError("the oracle answered the getter")


def check_render_multi(be, case, ref, render_multi=B.render_multi):
    p = case.params()
    hs = case.scene()
    with be.scene(hs) as s0, be.scene(hs) as s1:
        case.apply(s0)
        case.apply(s1)
        is_reference(case, render_multi(be, [s0, s1], p), ref, "equal settings")
        for other in case.multi_unequal:
            other(s1)
            refused(lambda: render_multi(be, [s0, s1], p), _abi.JADE_ERR_INVALID, (case.multi_words,))
        if case.multi_unset:
            case.multi_unset(s0)
            case.multi_unset(s1)
            render_multi(be, [s0, s1], p)


def check_refusal_leaves_the_handle_usable(be, case, ref):
    p = case.params()
    with be.scene(case.scene()) as sc:
        for step in case.usable:
            if step[0] == "do":
                step[1](sc)
            elif step[0] == "refused":
                refused((lambda: sc.begin(p)) if step[1] == "begin" else (lambda: sc.render(p)), _abi.JADE_ERR_UNSUPPORTED, step[2])
            elif step[0] == "reference":
                is_reference(case, sc.render(p), ref, "the refusals left the handle usable")
            elif step[0] == "finite":
                assert np.isfinite(sc.render(p)[0]).all()
            else:
                raise ValueError(step)


def check_command_line(case, tmp_path):
    """The flag renders and names the mode on the Start... line; each refused set of flags ends with exit code 2 and its words."""
    out = tmp_path / "mode.ppm"
    base = [CLI] + _CLI_BASE
    r = subprocess.run(base + case.cli["flags"] + ["--out", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    start = [ln for ln in r.stdout.splitlines() if ln.startswith("Start...")]
    assert len(start) == 1 and start[0].endswith(case.cli["suffix"]) and out.exists(), r.stdout
    for flags, words in case.cli["refused"]:
        r = subprocess.run(base + flags + ["--out", str(out)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and all(w in r.stderr for w in words), (flags, r.returncode, r.stderr)
