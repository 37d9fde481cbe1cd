"""Exposure (include/jade_bvh.h: jade_render_meter, jade_render_resolve_exposed, jade_expose_image): what DESIGN.md 3.7 quotes.

usage: python tools/exposure_ab.py --profile           the launches to take under `rocprofv3 --kernel-trace --stats` (no counters):
                                                       C3 at 1080p, 64 spp, then jade_render_resolve_ex, an automatic
                                                       jade_render_resolve_exposed, and jade_expose_image (meter only) on a 1080p
                                                       frame of one constant value and on a random one - in this order, so the first
                                                       k_meter<false> of the kernel trace is the contention case, the second the spread one
       python tools/exposure_ab.py [--out profiles/exposure_ab.json]
                                                       the exposure the defaults choose on C2 (512^2), C3, C3G (1080p) and C3 under the
                                                       procedural sky with its sun, 64 spp each; wall times of the calls
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import jaderaytracerendering_amd as J  # noqa: E402
from jaderaytracerendering_amd import _abi, backend as B  # noqa: E402

SPP = 64
FRAMES = (("C2", "C2", 512, 512, False), ("C3", "C3", 1920, 1080, False), ("C3G", "C3G", 1920, 1080, False),
          ("C3 + sky", "C3", 1920, 1080, True))


def scene(config, sky):
    b = J.SceneBuilder()
    try:
        cfg = b.config(config)
        if sky:
            b.set_env_sky()
        return b.build(), cfg
    finally:
        b.close()


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def contention_frames():
    rng = np.random.default_rng(3)
    const = np.full((1080, 1920, 3), 0.7, np.float32)
    rnd = (rng.random((1080, 1920, 3)) * 10.0 ** rng.uniform(-6, 4, (1080, 1920, 1))).astype(np.float32)
    return const, rnd


def profile():
    hip = J.hip()
    hs, cfg = scene("C3", False)
    p = B.params_from_config(cfg, spp=SPP, walk=_abi.WALK_EARLY_EXIT)
    p.width, p.height = 1920, 1080
    with hip.scene(hs) as sc:
        sc.begin(p)
        sc.flush(sc.step(SPP))
        sc.resolve(tonemap=_abi.TONEMAP_ACES)
        _, _, e, m = sc.resolve(exposure="auto")
    print(f"C3 1080p {SPP} spp: exposure {e!r}, {m}")
    for name, frame in zip(("constant", "random"), contention_frames()):
        _, _, m = hip.expose_image(frame, want_bgr8=False)
        print(name, m, "occupied bins:", int((m.bins > 0).sum()))


def defaults(out_path):
    hip = J.hip()
    d = hip.display_defaults()
    d.exposure_mode = _abi.EXPOSURE_AUTO
    res = {"what": __doc__.strip().splitlines()[0], "spp": SPP, "display": {k: getattr(d, k) for k, _ in _abi.DisplayParams._fields_},
           "frames": {}}
    for name, config, w, h, sky in FRAMES:
        hs, cfg = scene(config, sky)
        p = B.params_from_config(cfg, spp=SPP, walk=_abi.WALK_EARLY_EXIT)
        p.width, p.height = w, h
        with hip.scene(hs) as sc:
            sc.begin(p)
            sc.flush(sc.step(SPP))
            (rgb, bgr0), resolve_ms = timed(lambda: sc.resolve(tonemap=_abi.TONEMAP_ACES))
            sc.resolve(exposure=d)  # warm-up: first use allocates the meter's rows
            (_, bgr, e, m), exposed_ms = timed(lambda: sc.resolve(exposure=d))
            _, meter_ms = timed(sc.meter)
        full = hip.display_defaults()
        full.exposure_mode, full.p_lo, full.p_hi = _abi.EXPOSURE_AUTO, 0.0, 1.0
        occupied = np.flatnonzero(m.bins)
        res["frames"][name] = dict(
            config=config, width=w, height=h, sky=sky, exposure=e, ev=float(np.log2(e)), exposure_full_window=hip.meter_exposure(m, full),
            lum_min=float(m.lum_min), lum_max=float(m.lum_max), n_positive=m.n_positive, n_zero=m.n_zero, n_negative=m.n_negative,
            n_nonfinite=m.n_nonfinite, bins_occupied=int(len(occupied)), first_bin=int(occupied[0]), last_bin=int(occupied[-1]),
            bytes_255_share_unexposed=float((bgr0 == 255).mean()), bytes_255_share_exposed=float((bgr == 255).mean()),
            bytes_0_share_unexposed=float((bgr0 == 0).mean()), bytes_0_share_exposed=float((bgr == 0).mean()),
            mean_byte_unexposed=float(bgr0.mean()), mean_byte_exposed=float(bgr.mean()),
            resolve_ex_wall_ms=resolve_ms, resolve_exposed_wall_ms=exposed_ms, meter_wall_ms=meter_ms)
        print(name, json.dumps(res["frames"][name]), flush=True)
    const, rnd = contention_frames()
    hip.expose_image(const[:16, :16], want_bgr8=False)
    for name, frame in (("constant", const), ("random", rnd)):
        (_, _, m), ms = timed(lambda: hip.expose_image(frame, want_bgr8=False))
        res["frames"]["1080p " + name] = dict(expose_image_meter_only_wall_ms=ms, bins_occupied=int((m.bins > 0).sum()))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exposure_ab.json"))
    a = ap.parse_args()
    if a.profile:
        profile()
    else:
        defaults(a.out)


if __name__ == "__main__":
    main()
