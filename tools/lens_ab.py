"""Thin lens (include/jade_bvh.h: jade_scene_set_lens): what DESIGN.md 3.9 quotes.

usage: python tools/lens_ab.py [--out profiles/lens_ab.json] [--spp 1024] [--repeats 3]
           C3 at 1080p, one step of --spp samples plus flush, three ways: under a lens focused on the statue (autofocus on the frame's
           centre) whose aperture blurs the deepest point in view by about 10 pixels; the pinhole under JADE_FUSED=0 JADE_TAIL=0 - the
           lens's own schedule, with the parent's kernels; the pinhole under the default schedule.  Each way in a scene handle of its own
           (the switches are read at jade_scene_create), --repeats times, device times from jade_stats.
       python tools/lens_ab.py --picture profiles/images [--config C3]
           the configuration at 480 x 270, 256 spp, with and without that lens, as PNG
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

WIDTH, HEIGHT = 1920, 1080
BLUR_PX = 10.0
SWITCHES = ("JADE_FUSED", "JADE_TAIL")


def built(config):
    b = J.SceneBuilder()
    try:
        cfg = b.config(config)
        hs = b.build()
    finally:
        b.close()
    return hs, cfg


def choose_lens(sc, p):
    """Focus on the frame's centre; the aperture that blurs the deepest surface seen on a 24 x 14 grid of pixels by BLUR_PX pixels:
    R_px = 0.75 height A |1/z - 1/f| (include/jade_bvh.h)."""
    f = sc.focus_distance(p, p.width // 2, p.height // 2)
    z_far = f
    for gy in range(14):
        for gx in range(24):
            try:
                z_far = max(z_far, sc.focus_distance(p, (2 * gx + 1) * p.width // 48, (2 * gy + 1) * p.height // 28))
            except RuntimeError:  # the sky
                pass
    A = BLUR_PX / (0.75 * p.height * abs(1.0 / z_far - 1.0 / f))
    return float(A), float(f), float(z_far)


def one_way(hip, hs, p, lens, env, spp, repeats):
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)
    runs = []
    with hip.scene(hs) as sc:
        if lens:
            sc.set_lens(*lens)
        for _ in range(repeats + 1):  # the first allocates: left out
            st = _abi.Stats()
            t0 = time.perf_counter()
            sc.begin(p)
            sc.step(spp, st)
            sc.flush(st)
            wall = (time.perf_counter() - t0) * 1e3
            shade = st.kernel_ms - st.trace_ms - st.light_ms - st.tail_ms
            runs.append(dict(wall_ms=wall, kernel_ms=st.kernel_ms, k_trace_ms=st.trace_ms, first_pass_ms=st.light_ms, k_tail_ms=st.tail_ms,
                             shading_and_rest_ms=shade, rays=st.rays, rays_primary=st.rays_primary, rays_inline=st.rays_inline,
                             nodes_visited=st.nodes_visited, trace_launches=st.trace_launches, mray_per_s=st.rays / st.kernel_ms / 1e3))
    for k in SWITCHES:
        os.environ.pop(k, None)
    runs = runs[1:]
    best = min(runs, key=lambda r: r["kernel_ms"])
    return dict(env=env, lens=lens, runs=runs, kernel_ms_median=float(np.median([r["kernel_ms"] for r in runs])), fastest=best)


def measure(out_path, spp, repeats):
    hip = J.hip()
    hs, cfg = built("C3")
    p = B.params_from_config(cfg, spp=spp, walk=_abi.WALK_EARLY_EXIT)
    p.width, p.height = WIDTH, HEIGHT
    with hip.scene(hs) as sc:
        A, f, z_far = choose_lens(sc, p)
    res = {"what": __doc__.strip().splitlines()[0], "config": "C3", "width": WIDTH, "height": HEIGHT, "spp": spp, "repeats": repeats,
           "lens": dict(aperture_radius=A, focus_distance=f, deepest_point_in_view=z_far, its_blur_px=BLUR_PX), "ways": {}}
    res["ways"]["lens"] = one_way(hip, hs, p, (A, f), {}, spp, repeats)
    res["ways"]["pinhole, the lens's schedule (JADE_FUSED=0 JADE_TAIL=0)"] = one_way(hip, hs, p, None, {"JADE_FUSED": "0", "JADE_TAIL": "0"}, spp, repeats)
    res["ways"]["pinhole, default schedule"] = one_way(hip, hs, p, None, {}, spp, repeats)
    for k, v in res["ways"].items():
        b = v["fastest"]
        print(f"{k}: kernel {v['kernel_ms_median']:.1f} ms median ({', '.join('%.1f' % r['kernel_ms'] for r in v['runs'])}); fastest: k_trace "
              f"{b['k_trace_ms']:.1f}, first pass {b['first_pass_ms']:.1f}, k_tail {b['k_tail_ms']:.1f}, shading and rest {b['shading_and_rest_ms']:.1f} ms; "
              f"{b['rays'] / 1e9:.3f} Grays, {b['mray_per_s']:.0f} Mray/s, {b['nodes_visited'] / b['rays']:.1f} nodes per ray", flush=True)
    print(json.dumps(res["lens"]))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fo:
        json.dump(res, fo, indent=1)
    print("wrote", out_path)


def picture(out_dir, config):
    from PIL import Image
    hip = J.hip()
    hs, cfg = built(config)
    p = B.params_from_config(cfg, spp=256, walk=_abi.WALK_EARLY_EXIT)
    p.width, p.height = 480, 270
    os.makedirs(out_dir, exist_ok=True)
    with hip.scene(hs) as sc:
        A, f, z_far = choose_lens(sc, p)
        A *= p.height / HEIGHT  # choose_lens aims at BLUR_PX pixels of THIS frame: the measured frame's aperture blurs by the same share of the height
        for name, lens in (("pinhole", None), ("lens", (A, f))):
            sc.set_lens(*lens) if lens else sc.set_lens(None)
            _, bgr, _ = sc.render(p, want_rgb=False)
            path = os.path.join(out_dir, f"{config}_{p.width}x{p.height}_{p.spp}spp_{name}.png")
            Image.fromarray(np.ascontiguousarray(bgr[::-1, :, ::-1])).save(path, optimize=True)  # row 0 = the bottom row; B G R
            print("wrote", path, os.path.getsize(path), "bytes", f"(aperture {A:.4g}, focus {f:.4g})" if lens else "")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lens_ab.json"))
    ap.add_argument("--spp", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--picture", metavar="DIR", default=None)
    ap.add_argument("--config", default="C3")
    a = ap.parse_args()
    if a.picture:
        picture(a.picture, a.config)
    else:
        measure(a.out, a.spp, a.repeats)


if __name__ == "__main__":
    main()
