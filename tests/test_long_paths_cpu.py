"""The committed long paths (tests/golden/long_paths.json, made by tools/find_long_paths.py) are what tests/long_paths.py says they
are - on the CPU: the stream model, the oracle, and the float64 statement of tests/jade_spec.py agree on every recorded sample.

What the GPU tests (test_gpu_long_paths.py) rest on is established here, as conditions on the fixtures and not as measurements:
every scene has at least 4 samples of JADE_STACK_CAPACITY pushes; in the lit and the mixed room at least 3 of them end in a term -
the last bounce's l_dir, counted a second time through the last rate - above 1e-3 of the sample, so that a module that drops or
mishandles it misses the pixel's bound; the pane room has at least 4 exhausted refraction loops and the mixed room at least 2."""
import numpy as np
import pytest

import jade_spec
import long_paths as LP
from conftest import COUNTER_KEYS, counters

CAPS_ALONE = LP.recorded("cap", ("alone",))
CHAINS_ALONE = LP.recorded("chain", ("alone",))
EVERY = LP.recorded("cap") + LP.recorded("chain")


def _id(item):
    name, r = item
    return f"{name}-{r['place']}-{r['frame']}"


_open = {}


def oracle_scene(oracle, name):
    if name not in _open:
        _open[name] = oracle.scene(LP.scene(name))
    return _open[name]


def test_stream_model_is_the_modules_generator(fpm):
    """wang / to_float / seed_of against include/jade_fpmath.h (tests/native/fpmath_export.c) and jade_spec.wang_stream; frame_for
    inverts the seed for any pixel and sample."""
    rng = np.random.default_rng(7)
    for x, y, frame in rng.integers(0, 2 ** 31, (20, 3)):
        x, y, frame = int(x) % 4096, int(y) % 4096, int(frame)
        seed = LP.seed_of(x, y, frame)
        assert seed == fpm.t_seed(x, y, frame)
        s, ws = np.uint32(seed), jade_spec.wang_stream(x, y, frame)
        with np.errstate(over="ignore"):
            for _ in range(8):
                s = LP.wang(s)
                assert float(LP.to_float(s)) == next(ws)
    for seed in (1, 71141, 0xffffffff, 0x80000001):
        for x, y, s in ((0, 0, 0), (5, 2, 0), (29, 13, 1), (4095, 4095, 3)):
            assert LP.seed_of(x, y, (LP.frame_for(seed, x, y, s) + s) & 0xffffffff) == seed


def test_the_sieve_finds_what_the_draws_say():
    """cap_seeds keeps exactly the seeds whose roulette draws all pass (a small range, a short path: a few of many)."""
    per, rr = LP.LAYOUTS["lit"]
    kept = LP.cap_seeds(per, rr, 1, 4000, bounces=24)
    draws = LP.roulette_draws(np.arange(4000, dtype=np.uint32) * 2 + 1, per, rr, 24)
    want = [int(2 * i + 1) for i in np.flatnonzero((draws < LP.RR).all(1))]
    assert kept == want and 100 < len(kept) < 1000


@pytest.mark.parametrize("item", [it for it in LP.recorded("cap") if it[0] in LP.LAYOUTS], ids=_id)
def test_stream_model_predicts_the_roulette_draws(item):
    """Where the layout of a bounce is fixed: the recorded seed is the sample's, and its first 128 roulette draws pass."""
    name, r = item
    pl = LP.PLACEMENTS[r["place"]]
    assert LP.seed_of(pl["x"], pl["y"], (r["frame"] + pl["s"]) & 0xffffffff) == r["seed"]
    draws = LP.roulette_draws([r["seed"]], *LP.LAYOUTS[name], LP.CAP)
    assert (draws < LP.RR).all()


@pytest.mark.parametrize("item", EVERY, ids=_id)
def test_oracle_has_the_recorded_lengths(oracle, item):
    """Every placement: the probe gives the recorded pushes, refraction rays and exhausted loops; alone in its frame, the render
    has the recorded counters - 128 pushes are 128 shaded vertices, each with its continuation ray traced."""
    name, r = item
    pl = LP.PLACEMENTS[r["place"]]
    so = oracle_scene(oracle, name)
    p = LP.params(name, r["place"], r["frame"])
    pushes, refr, chains = (int(v[0]) for v in LP.path_lengths(so, p, pl["x"], pl["y"], r["frame"] + pl["s"], 1))
    assert (pushes, refr, chains) == (r["pushes"], r["refract_rays"], r["chains"])
    n, l_dir, sd, sr, color = LP.path_probe(so, p, pl["x"], pl["y"], pl["s"])
    assert n == pushes and len(sd) == pushes
    if r["place"] == "alone":
        rgb, _, st = so.render(p)
        c = counters(st)
        assert c == r["counters"] and set(c) == set(COUNTER_KEYS)
        assert np.array_equal(rgb[0, 0].view(np.uint32), color.view(np.uint32)), "the probe's sample is not the render's"
        if pushes == LP.CAP:
            assert c["shaded_hits"] == LP.CAP and c["samples"] == 1
            # every push follows a continuation ray that was traced and hit: indirect, mirror, or a refraction's exit ray
            assert c["rays_indirect"] + c["rays_mirror"] + c["rays_refract"] >= LP.CAP
            if name == "mirror":
                assert c["rays_mirror"] == LP.CAP and c["rays_secondary"] == LP.CAP
            if name == "lit":
                assert c["rays_indirect"] == LP.CAP and c["rays_shadow"] == 2 * LP.CAP and c["rays_env"] == LP.CAP
    if item in LP.recorded("chain"):
        assert chains >= 1
        if name == "pane":
            assert refr == 33 * chains, "a loop that ran out is 32 rays and the exit ray"


@pytest.mark.parametrize("item", CAPS_ALONE + CHAINS_ALONE, ids=_id)
def test_float64_statement_stops_at_the_same_depth(item):
    name, r = item
    info = {}
    eye, cam = LP.camera(name)
    jade_spec.sample(_spec(name), 0, 0, 1, 1, eye, cam, r["frame"], None, info)
    assert info["pushes"] == r["pushes"] and info["chains"] == r["chains"]


_specs = {}


def _spec(name):
    if name not in _specs:
        _specs[name] = jade_spec.Scene(LP.scene(name))
    return _specs[name]


@pytest.mark.parametrize("item", CAPS_ALONE, ids=_id)
def test_both_orders_of_summation_are_within_the_bound(oracle, item):
    """From the exported stacks: the reference's Horner unwinding and the module's forward sum, each in float32, are within
    2 n u A of the exact sum (n = pushes + 1 terms, each through at most n roundings of relative size u: (1 + u)^(2n) - 1 < 2 n u
    (1 + 2 n u) per term, against the sum of the absolute terms A; 2 n u = 1.5e-5 here, so the second order is below the first's
    thousandth) - which is why the two may differ by 4 n u A on a pixel and no more.  The Horner value is the oracle's own."""
    name, r = item
    so = oracle_scene(oracle, name)
    p = LP.params(name, "alone", r["frame"])
    n, l_dir, sd, sr, color = LP.path_probe(so, p, 0, 0, 0)
    q = LP.sums(l_dir, sd, sr)
    assert q["n"] == LP.CAP + 1
    assert np.array_equal(q["horner"].view(np.uint32), color.view(np.uint32)), "the unwinding restated in numpy is not the oracle's"
    bound = 2 * q["n"] * LP.U * q["A"] * (1 + 1e-3)
    for what in ("horner", "forward"):
        err = np.abs(q[what].astype(np.float64) - q["exact"])
        print(f"{name} {r['frame']}: {what} off by {err.max():.3g}, bound {bound.max():.3g}, share of the last term {r['last_share']:.3g}")
        assert (err <= bound).all(), what
    share = float(np.max(np.abs(q["last"])) / max(float(np.max(np.abs(color))), 1e-300))
    assert share == pytest.approx(r["last_share"], rel=1e-9, abs=1e-300)


def test_conditions_on_the_fixtures():
    fx = LP.fixtures()
    for name in LP.SCENES:
        caps = [r for r in fx[name]["cap"] if r["pushes"] == LP.CAP]
        assert len([r for r in caps if r["place"] == "alone"]) >= 4, name
        assert {r["place"] for r in caps} == set(LP.PLACEMENTS), name
        assert fx[name]["triangles"] == LP.scene(name).n_triangles <= 28
    for name in ("lit", "mixed"):
        visible = [r for r in fx[name]["cap"] if r["place"] == "alone" and r["last_share"] > 1e-3]
        assert len(visible) >= 3, (name, [r["last_share"] for r in fx[name]["cap"] if r["place"] == "alone"])
    assert len([r for r in fx["pane"]["chain"] if r["chains"] >= 1]) >= 4
    assert len([r for r in fx["mixed"]["chain"] if r["chains"] >= 1]) >= 2
    # the mixed room's cap is reached through several kinds of push, the refraction exit among them
    kinds = [r["counters"] for r in fx["mixed"]["cap"] if r["place"] == "alone"]
    assert sum(c["rays_refract"] > 0 and c["rays_mirror"] > 0 and c["rays_indirect"] > 0 for c in kinds) >= 2
