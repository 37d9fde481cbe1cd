"""tests/mode_seams.py can fail: every check, for every case of its table, against a numpy stand-in for a backend - which passes - and
against stand-ins that are wrong in one way each, which the corresponding check must catch with an AssertionError.  A guard against a
suite that silently checks nothing, not a second renderer: the stand-in's frame and counters are a pure function of the scene, the
parameters, the settings at begin and the tile share.  check_command_line starts the command-line tool and is not run here."""
import os
import zlib

import numpy as np
import pytest

import mode_seams as MS
from jaderaytracerendering_amd import _abi, backend as B

CAUGHT_BY = {"mode at flush": "steps", "shares overlap": "shares", "loses a shadow ray": "schedules", "accepts unknown": "unknown value",
             "cached bit": "walks"}  # a stand-in's fault: the check that must catch it
FAULTS = tuple(CAUGHT_BY)


def _refuse(code, text):
    raise B.JadeError(code, text)


class Scene:
    def __init__(self, be, hs):
        self.be, self.key = be, (int(hs.n_triangles), len(hs.a["emit"]))
        self.env = {k: v for k, v in os.environ.items() if k.startswith("JADE_")}  # (read once, at creation)
        self.set = dict(lens=(0.0, 0.0), shutter=None, light=0, bounce=0, direct=0)
        self.cached_renders = 0

    def __enter__(self):
        return self

    def __exit__(self, *a):
        pass

    # ---- the settings
    def set_lens(self, a, f=0.0):
        self.set["lens"] = (float(a), float(f)) if a else (0.0, 0.0)

    def lens(self):
        return self.set["lens"]

    def set_shutter(self, eye, cam=None, t0=0.0, t1=1.0):
        self.set["shutter"] = None if eye is None else (np.float32(eye).tobytes(), np.float32(cam).tobytes(), float(t0), float(t1))

    def shutter(self):
        return self.set["shutter"]

    def _mode(self, name, value):
        if value not in (0, 1) and "accepts unknown" not in self.be.faults:
            _refuse(_abi.JADE_ERR_INVALID, f"unknown {name} sampling")
        self.set[name] = value

    light_sampling = property(lambda self: self.set["light"])
    bounce_sampling = property(lambda self: self.set["bounce"])
    direct_sampling = property(lambda self: self.set["direct"])
    set_light_sampling = lambda self, v: self._mode("light", v)  # noqa: E731
    set_bounce_sampling = lambda self, v: self._mode("bounce", v)  # noqa: E731
    set_direct_sampling = lambda self, v: self._mode("direct", v)  # noqa: E731

    # ---- a render
    def begin(self, p):
        s = self.set
        camera = " and ".join(w for w, on in (("a lens", s["lens"][0] > 0), ("a shutter", s["shutter"] is not None)) if on)
        if camera and s["light"]:
            _refuse(_abi.JADE_ERR_UNSUPPORTED, "light sampling: JADE_LIGHTS_ONE does not run together with " + camera)
        if camera and s["bounce"]:
            _refuse(_abi.JADE_ERR_UNSUPPORTED, "bounce sampling: JADE_BOUNCE_COSINE does not run together with " + camera)
        if s["direct"] and not s["bounce"]:
            _refuse(_abi.JADE_ERR_UNSUPPORTED, "direct sampling: JADE_DIRECT_MIS needs JADE_BOUNCE_COSINE")
        self.p, self.done, self.began = type(p).from_buffer_copy(p), 0, dict(s)

    def _owned(self):
        """[H, W] bool: the pixels of this share's 16 x 16 tiles."""
        p = self.p
        ty, tx = np.mgrid[0:p.height, 0:p.width] // 16
        own = (ty * ((p.width + 15) // 16) + tx) % p.tile_nranks == p.tile_rank
        if "shares overlap" in self.be.faults and p.tile_rank == 1:
            own[0, 0] = True
        return own

    def step(self, n, st=None):
        st = st if st is not None else _abi.Stats()
        self.done += n
        k = int(self._owned().sum()) * n
        sampling = self.began["light"] or self.began["bounce"] or self.began["direct"]
        read = {_abi.WALK_REFERENCE: 10, _abi.WALK_EARLY_EXIT: 7, _abi.WALK_EARLY_EXIT_CACHED: 8}[self.p.walk]
        add = dict(samples=k, rays_primary=k, shaded_hits=k, rays_shadow=2 * k, rays_env=k, rays_indirect=k, rays_mirror=k, rays_refract=0,
                   rays_secondary=5 * k, nodes_visited=read * k, tris_tested=read * k, rays_inline=k if sampling else 0,
                   rays_cached=k if self.p.walk == _abi.WALK_EARLY_EXIT_CACHED else 0)
        for name, v in add.items():
            setattr(st, name, getattr(st, name) + v)
        return st

    def flush(self, st=None):
        if "mode at flush" in self.be.faults:
            self.began = dict(self.set)
        if st is not None and "loses a shadow ray" in self.be.faults and self.env.get("JADE_SORT") == "1":
            st.rays_shadow -= 1
        return st

    def resolve(self):
        p, seed = self.p, zlib.crc32(repr((self.key, sorted(self.began.items()), self.p.frame, self.done)).encode())
        y, x, c = np.mgrid[0:p.height, 0:p.width, 0:3]
        rgb = (1 + (x * 7 + y * 13 + c * 29 + seed) % 1000).astype(np.float32) / np.float32(8)
        rgb[~self._owned()] = 0
        return rgb, rgb.astype(np.uint8)

    def render(self, p):
        self.begin(p)
        st = self.step(p.spp)
        self.flush(st)
        rgb, bgr = self.resolve()
        if p.walk == _abi.WALK_EARLY_EXIT_CACHED:
            self.cached_renders += 1
            if "cached bit" in self.be.faults and self.cached_renders == 2:
                rgb.view(np.uint32)[3, 5, 1] ^= 1
        return rgb, bgr, st

    def query(self, what):
        assert what == _abi.Q_RECORDS_PER_PIXEL
        return int(self.env.get("JADE_RECORDS_PER_PIXEL", 8))


class StandIn:
    def __init__(self, *faults):
        assert set(faults) <= set(FAULTS)
        self.faults = faults

    def scene(self, hs):
        return Scene(self, hs)


def render_multi(be, scenes, p):
    s0 = scenes[0]
    for key, noun in (("lens", "lenses"), ("shutter", "shutters"), ("light", "light sampling modes"), ("bounce", "bounce sampling modes"),
                      ("direct", "direct sampling modes")):
        if any(s.set[key] != s0.set[key] for s in scenes):
            _refuse(_abi.JADE_ERR_INVALID, f"the scenes carry different {noun}")
    return s0.render(p)


class Oracle:
    """Refuses every setter and getter of a mode, as oracle/libjade_oracle.so does."""
    class _Scene(Scene):
        def __getattribute__(self, name):
            if name.startswith(("set_", "lens", "shutter")) or name.endswith("_sampling"):
                _refuse(_abi.JADE_ERR_UNSUPPORTED, "the oracle has no such entry point")
            return object.__getattribute__(self, name)

    faults = ()

    def scene(self, hs):
        return self._Scene(self, hs)


# what runs one check of a case against a stand-in; the schedules check runs every environment of the case
def _run_schedules(be, case, ref, monkeypatch):
    for env in MS.schedules(case):
        with monkeypatch.context() as m:
            MS.check_schedule(be, case, ref, env, m.setenv)


CHECKS = {
    "twice": lambda be, case, ref, mp: MS.check_twice(be, case, ref),
    "walks": lambda be, case, ref, mp: MS.check_walks(be, case, ref),
    "steps": lambda be, case, ref, mp: MS.check_steps(be, case, ref),
    "shares": lambda be, case, ref, mp: MS.check_shares(be, case, ref),
    "schedules": _run_schedules,
    "unknown value": lambda be, case, ref, mp: MS.check_unknown_value(be, case) if case.knob else None,
    "render_multi": lambda be, case, ref, mp: MS.check_render_multi(be, case, ref, render_multi=render_multi),
    "usable": lambda be, case, ref, mp: MS.check_refusal_leaves_the_handle_usable(be, case, ref) if case.usable else None,
}


def test_the_table_has_the_six_cases_and_every_list_holds_the_common_one():
    assert [c.name for c in MS.CASES] == ["lens", "shutter", "shutter+lens", "one-light", "cosine", "MIS"]
    assert MS.SAMPLING == ["one-light", "cosine", "MIS"]
    assert len(MS.COMMON_SCHEDULES) == 7
    for case in MS.CASES:
        envs = MS.schedules(case)
        assert envs and all(env in envs for env in MS.COMMON_SCHEDULES), case.name
        assert len({MS.schedule_id(e) for e in envs}) == len(envs), "no environment twice"
        n, spp = case.steps
        assert n * spp == case.params().spp and case.shares in (2, 3)
    assert all(len(MS.schedules(MS.BY_NAME[c])) == 22 for c in ("lens", "shutter", "shutter+lens"))


@pytest.mark.parametrize("case", [c.name for c in MS.CASES])
def test_the_stand_in_passes_every_check(case, monkeypatch):
    case, be = MS.BY_NAME[case], StandIn()
    ref = MS.reference(be, case)
    for name, check in CHECKS.items():
        check(be, case, ref, monkeypatch)
    MS.check_oracle_refuses(Oracle(), case)
    with pytest.raises(AssertionError):
        MS.check_oracle_refuses(be, case)  # (the stand-in answers: not an oracle)


# (the camera modes have no setter that takes a mode's value)
@pytest.mark.parametrize("case,fault", [(c.name, f) for c in MS.CASES for f in FAULTS if c.knob or f != "accepts unknown"])
def test_a_wrong_stand_in_is_caught_by_its_check(case, fault, monkeypatch):
    case, be = MS.BY_NAME[case], StandIn(fault)
    ref = MS.reference(be, case)
    with pytest.raises(AssertionError):
        CHECKS[CAUGHT_BY[fault]](be, case, ref, monkeypatch)
