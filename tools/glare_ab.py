"""Glare (include/jade_bvh.h: jade_glare_image, jade_render_glare): what DESIGN.md 3.8 quotes.

usage: python tools/glare_ab.py --profile              the launches to take under `rocprofv3 --kernel-trace --stats` (no counters):
                                                       C3 at 1080p, 64 spp, then five jade_render_glare at the defaults (6 levels)
       python tools/glare_ab.py [--out profiles/glare_ab.json]
                                                       on that render: wall times of jade_render_glare and jade_glare_image at 1, 3, 6
                                                       and 9 levels beside jade_render_resolve_exposed (medians of 7 calls after a
                                                       warm-up, which allocates), and what the defaults do to the frame's bytes
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

SPP, WIDTH, HEIGHT = 64, 1920, 1080
LEVELS = (1, 3, 6, 9)
REPEATS = 7


def rendered(hip, config="C3"):
    b = J.SceneBuilder()
    try:
        cfg = b.config(config)
        hs = b.build()
    finally:
        b.close()
    p = B.params_from_config(cfg, spp=SPP, walk=_abi.WALK_EARLY_EXIT)
    p.width, p.height = WIDTH, HEIGHT
    sc = hip.scene(hs)
    sc.begin(p)
    sc.flush(sc.step(SPP))
    return sc


def median_ms(fn):
    fn()  # warm-up: first use allocates
    times = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), float(min(times))


def profile():
    hip = J.hip()
    with rendered(hip) as sc:
        for _ in range(5):
            _, _, e = sc.glare()
    print(f"C3 {WIDTH}x{HEIGHT} {SPP} spp, glare defaults, exposure {e!r}")


def measure(out_path):
    hip = J.hip()
    gp = hip.glare_defaults()
    auto = hip.display_defaults()
    auto.exposure_mode = _abi.EXPOSURE_AUTO
    res = {"what": __doc__.strip().splitlines()[0], "config": "C3", "width": WIDTH, "height": HEIGHT, "spp": SPP, "repeats": REPEATS,
           "defaults": {k: getattr(gp, k) for k, _ in _abi.GlareParams._fields_}, "wall_ms": {}}
    with rendered(hip) as sc:
        rgb0, bgr0 = sc.resolve(tonemap=_abi.TONEMAP_ACES)
        res["wall_ms"]["jade_render_resolve_ex"] = median_ms(lambda: sc.resolve(tonemap=_abi.TONEMAP_ACES))
        res["wall_ms"]["jade_render_resolve_exposed manual"] = median_ms(lambda: sc.resolve(exposure=1.0))
        res["wall_ms"]["jade_render_resolve_exposed auto"] = median_ms(lambda: sc.resolve(exposure=auto))
        for levels in LEVELS:
            p = hip.glare_defaults()
            p.levels = levels
            res["wall_ms"][f"jade_render_glare {levels} levels manual"] = median_ms(lambda: sc.glare(p))
            res["wall_ms"][f"jade_render_glare {levels} levels auto"] = median_ms(lambda: sc.glare(p, auto))
            res["wall_ms"][f"jade_render_glare {levels} levels bytes only"] = median_ms(lambda: sc.glare(p, want_rgb=False))
            res["wall_ms"][f"jade_glare_image {levels} levels"] = median_ms(lambda: hip.glare_image(rgb0, p))
        rgb, bgr, _ = sc.glare()
    lum = lambda a: 0.3 * a[..., 0].astype(np.float64) + 0.6 * a[..., 1] + 0.1 * a[..., 2]  # noqa: E731
    res["frame"] = dict(sum_ratio=[float(rgb[..., c].sum(dtype=np.float64) / rgb0[..., c].sum(dtype=np.float64)) for c in range(3)],
                        luminance_max_before=float(lum(rgb0).max()), luminance_max_after=float(lum(rgb).max()),
                        pixels_above_one_before=int((lum(rgb0) > 1).sum()), pixels_above_one_after=int((lum(rgb) > 1).sum()),
                        bytes_changed_share=float((bgr != bgr0).any(-1).mean()), bytes_255_share_before=float((bgr0 == 255).mean()),
                        bytes_255_share_after=float((bgr == 255).mean()))
    for k, v in res["wall_ms"].items():
        print(f"{k}: median {v[0]:.3f} ms, fastest {v[1]:.3f} ms", flush=True)
    print(json.dumps(res["frame"]))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "glare_ab.json"))
    a = ap.parse_args()
    if a.profile:
        profile()
    else:
        measure(a.out)


if __name__ == "__main__":
    main()
